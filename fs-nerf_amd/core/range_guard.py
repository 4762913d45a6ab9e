"""What follows when an fp16-mode launch of a NeRF reports values outside the mode's range envelope: the exponents of a
calibration, the state of the activation scaling and of training (with the periodic host look), the read-back disciplines
of a launch (sync, deferred, never).  The model keeps the knobs, the counters and `fall_back`, and is passed in."""
import math
import warnings
from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from .. import _lib as L
from .. import ops
from ..shard import max_bits_over_ranks

ENVELOPE = L.FSN_STATUS_FP16_RANGE | L.FSN_STATUS_FP16_SMALL


def choose_exponents(amax, wmax, target: int, old: Optional[list], keep_if_close: bool, n_layers: int) -> list:
    """The exponent of every GEMM (hidden layers, connection, branch) from the probe's largest |activation| `amax`
    (`NeRF.calibrate`); `old`: the exponents in force or None; `wmax`: largest |weight|, activation then encoding columns."""
    exps = []
    for g, v in enumerate(amax):
        if not math.isfinite(v):
            raise RuntimeError(f"NeRF.calibrate: layer {g} produced non-finite activations on the probe batch")
        if v <= 0.0:
            e = old[g] if old is not None else 0  # dead layer on the probe: its scale does not matter
        else:
            e = target - math.ceil(math.log2(v))
            if keep_if_close and old is not None and 2.0 ** (target - 3) <= v * 2.0 ** old[g] <= 2.0 ** (target + 1):
                e = old[g]
        exps.append(max(-60, min(60, e)))
    # scaled weights: W_g * 2^(e_g - e_prev) on activation columns, W_g * 2^e_g on encoding columns, below 2^15
    # (in GEMM order every GEMM reads its predecessor: the connection the last hidden layer, the branch the connection)
    for g in range(n_layers + 2):
        prev = exps[g - 1] if g else 0
        for wm, sh in ((wmax[2 * g], exps[g] - prev), (wmax[2 * g + 1], exps[g])):
            if wm > 0.0 and math.isfinite(wm):
                over = math.ceil(math.log2(wm)) + sh - 15
                if over > 0:
                    exps[g] -= over
    return exps


class PackCache:
    """A packed blob and its key: re-packed when the key is `stale`, into the same `PackedMLP` while mode and device match."""
    pm = key = None

    def stale(self, key) -> bool:
        return self.pm is None or key != self.key

    def pack(self, desc, prec: int, dev, key, ws, bs, exps=None) -> ops.PackedMLP:
        if self.pm is None or self.pm.prec != prec or self.pm.blob.device != dev:
            self.pm = ops.PackedMLP(desc, prec, dev)
        self.pm.pack(ws, bs, exps)
        self.key = key
        return self.pm


class ActScaling:
    """Per-layer activation scaling of fp16x3 inference: what `NeRF.calibrate` measured (nothing of it is in a state_dict)."""

    def __init__(self) -> None:
        self.exps: Optional[list] = None   # n_layers + 2 exponents (kernel GEMM order), None = not calibrated
        self.key = None                    # parameter versions the calibration was made with
        self.moves = 0                     # target moves since then (same weights, data did not fit)
        self.moved_by = 0                  # ... and their sum: undone when the weights change
        self.needs_calibration = False     # calibrate (with hysteresis) at the next pack
        self.blob = PackCache()            # the unscaled bf16x3 network of the probe launch

    def forget_target_moves(self, model) -> None:
        # target moves answered a probe that did not represent the data under the OLD weights
        model.act_target_exp -= self.moved_by
        self.moved_by = self.moves = 0

    def recalibrate(self, model, bits: int, probe) -> bool:
        """A scaled-mode launch reported that its calibration does not fit the data.  Other weights than the calibration
        saw: measure again.  Same weights: the probe was not representative - move the target (overflow: 2^4 more
        headroom; small: 2^3 less) and measure again, at most three times.  False: give up (bf16x3)."""
        if self.exps is not None and self.key == model._param_key():
            if self.moves >= 3 or bits == ENVELOPE:
                return False
            self.moves += 1
            move = -4 if bits & L.FSN_STATUS_FP16_RANGE else 3
            model.act_target_exp += move
            self.moved_by += move
            if not 2 <= model.act_target_exp <= 14:
                return False
        else:
            self.forget_target_moves(model)
        try:
            model.calibrate(probe)
        except RuntimeError:
            return False
        return True


class _Calls:
    """One kind of backward call: accumulated range words (device int32 [2]; OR of the calls' words since the last host
    look: [0] the training kernels', [1] the sampler's density pass), call counter, delayed stage scaling of the backward."""
    word = stage = None
    calls, calibrated = 0, False

    def word_on(self, dev) -> Tensor:
        if self.word is None or self.word.device != dev:
            self.word = torch.zeros(2, dtype=torch.int32, device=dev)
        return self.word

    def stage_on(self, dev, n: int) -> Tuple[Tensor, Tensor]:
        """(scales, maxima) of the backward chain's delayed per-stage scaling (fsn_nerf_train_bwd), device-resident."""
        if self.stage is None or self.stage[0].device != dev:
            self.stage = (torch.ones(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
            self.calibrated = False
        return self.stage


class TrainStatus:
    """`train`: training steps.  `inputs`: calls that compute input gradients only (a frozen network,
    `density_gradient`): their cotangents are other quantities, so they steer a pair of arrays of their own."""

    def __init__(self) -> None:
        self.train, self.inputs = _Calls(), _Calls()

    @staticmethod
    def step_flags(model, dev) -> list:
        """The step-flag words a training launch of this model reports into (device int32 [1] each): the word of every
        gradient bucket that owns one of its parameters (`shard.FlatGrads.step_flag`, consumed by that bucket's
        optimizer), and the device's shared word (`ops.step_flag`) for parameters no bucket owns."""
        flags, loose = {}, False
        for p in model.parameters():
            f = getattr(p, "_fsn_step_flag", None)
            if f is None or f.device != dev:
                loose = True
            else:
                flags[id(f)] = f
        out = list(flags.values())
        if loose or not out:
            out.append(ops.step_flag(dev))
        return out

    def fold(self, model, word: Tensor, dev, slot: int) -> None:
        """A training-time launch's range word (device int32 [1]) joins the step's guard on the device, no host sync: ORed
        into every step flag of this model (FusedAdam skips a flagged step) and into slot `slot` of `train`'s word."""
        for f in self.step_flags(model, dev):
            f.bitwise_or_(word)
        self.train.word_on(dev)[slot:slot + 1].bitwise_or_(word)

    def after_backward(self, model, word: Tensor, dev, step: bool) -> None:
        """A backward's range word (fp16 modes) and the host's periodic look; `step`: a training step, else input gradients."""
        # fp16 range guard without a per-step host sync.  When this call's launches reported values outside the fp16
        # range, the backward kernels have written ITS gradients as zeros on the device; the call's word is folded
        # (device ops) into the device's step flag, on which FusedAdam skips the whole update - a skipped step, like a
        # loss scaler's - and into this model's own accumulated word, which the host reads every `range_check_every`
        # training calls; it then warns and continues in bf16x3.
        # Range word of a backward that computed input gradients only (fp16 modes; its gradients are zeros when the
        # word is set).  Not a training step: it joins neither the optimizer's step flags nor `train.calls`; it is ORed
        # into a word of its own that the host reads every `range_check_every` such calls - a flagged one then warns and
        # the model continues in the bf16 mode, as after a flagged training step.
        kind = self.train if step else self.inputs
        if step:
            self.fold(model, word, dev, 0)
        else:
            kind.word_on(dev)[0:1].bitwise_or_(word)
        kind.calls += 1
        if not model.range_check or kind.calls % model.range_check_every != 0:
            return
        if step:
            model._guard_weights("training steps", training=True)
        # Host look at the accumulated words (one 8-byte read-back) and clear -> (training kernels' bits, sampler's
        # bits).  Data-parallel runs take the MAX over the ranks first (every rank makes the same number of training
        # calls, so all of them are here together): a rank that overflowed and one that did not must not continue in
        # different arithmetic.
        w = kind.word_on(dev)
        local, samp = (int(v) for v in w.tolist())
        if local & L.FSN_STATUS_GRAD_RANGE:  # delayed gradient scaling skipped a step (and lowered a stage): no fall-back
            model.grad_overflow_looks += 1
        bits, sampler_bits = local & ENVELOPE, samp & ENVELOPE
        if step:
            # (MAX of bit masks 0..3: both bits lead to the same action, so the largest mask is enough; the two words are
            # reduced separately - a MAX over a combined mask would lose the smaller word's bits)
            bits = max_bits_over_ranks(bits, dev)
            sampler_bits = max_bits_over_ranks(sampler_bits, dev)
        if local or samp or bits or sampler_bits:
            w.zero_()
        if bits:
            model.fall_back("training steps (an overflowing step's gradients were zeroed on the device and its optimizer "
                            "update skipped)" if step else
                            "input-gradient calls (a flagged call's gradients were written as zeros)", bits, scaled=False)
        # The sampler's density pass in front of the training forward is an INFERENCE launch (scaled fp16x3):
        # a flag there says its per-layer scales no longer fit the weights being trained (the step was skipped
        # on the device); the next sampler call re-calibrates on its own rays.  Also every 4th look, flag or
        # not, so that the scales follow the network long before a guard trips.
        if step and (sampler_bits or (kind.calls // model.range_check_every) % 4 == 0):
            model.act_state.needs_calibration = True


def sampler_launch(model, needs_grad: bool, dev, probe, launch):
    """`launch(packed, status=None)` of a fused sampler (its density pass is an inference launch of `model`).  Training
    step in a guarded fp16 mode: no host read-back between the sampler and the forward (it cost the step 0.2 ms of idle
    GPU); the sampler reports into a word of its own, which joins the step's guard on the device like the forward /
    backward pair's does (TrainStatus.fold): an overflowing density pass makes this a skipped step (FusedAdam); at its
    next periodic look the host re-calibrates the density pass's per-layer scales (scaled fp16x3 inference) or
    switches to bf16x3.  Otherwise the launch runs under the range guard."""
    with torch.no_grad():
        if needs_grad and model.fp16_mode and model.range_check:
            word = torch.zeros(1, dtype=torch.int32, device=dev)
            out = launch(model.packed(probe), status=word)
            model.train_state.fold(model, word, dev, 1)
            return out
        return guarded_launch([model], dev, "the sampler's density pass", probe, lambda: launch(model.packed(probe)))


def _warn_single_pass(model, what: str, bits: int) -> str:
    model.range_events += 1
    warnings.warn(f"fs-nerf HIP path: {what}: hidden activations left the fp16 range envelope of precision 'fp16' "
                  f"({ops.describe_flags(bits)}); re-running / continuing in 'bf16'", RuntimeWarning, stacklevel=4)
    return "bf16"


def single_pass_launch(model, precision: str, dev, what: str, leave_fp16, launch, undo=None):
    """`launch(packed blob)` in the opt-in single-pass mode `precision` under the fp16 range guard (`guarded_launch`'s
    policy for a mode that is not the model's own): "bf16" has float32's range and raises no flags - no host read;
    "fp16" reads the launch's word back (one host sync, unless `model.range_check` is False), and a flagged launch leaves
    no trace: `undo()`, `leave_fp16(what, bits)` (warns, moves its owner to "bf16" for good), and the call is made again
    in bf16."""
    out = launch(model.packed_single(precision))
    if precision == "fp16" and model.range_check:
        bits = ops.range_flags(dev)
        if bits:
            if undo is not None:
                undo()
            out = launch(model.packed_single(leave_fp16(what, bits)))
    return out


def guarded_launch(nets: Sequence, dev, what: str, probe, launch, earlier: str = "call"):
    """`launch()` under the fp16 range guard for the NeRFs `nets` it evaluates (one precision mode for all of them).
    range_check True: read the launch's word back (one host sync); a flagged call is re-run after `fall_back`
    (re-calibration of the scaled fp16x3 path, or bf16x3).  "deferred": no wait - the word of the PREVIOUS launch is
    looked at now (a raised flag re-calibrates / switches the nets and says that the previous call's outputs are
    invalid), this launch posts its own for the next call / `frame_flagged` to look at.  False: never look."""
    guarded = [m for m in nets if m.range_check and m.fp16_mode]
    if guarded and all(m.range_check == "deferred" for m in guarded):
        bits = ops.range_poll(dev)
        if bits:
            _fall_back(nets, f"an EARLIER {earlier} (deferred range check: its outputs are invalid)", bits, probe, True)
        out = launch()
        if any(m.fp16_mode for m in nets):
            ops.range_post(dev)
        return out
    out = launch()
    for _ in range(5):
        bits = ops.range_flags(dev) if guarded else 0
        if not bits:
            break
        _fall_back(nets, what, bits, probe)
        out = launch()
        guarded = [m for m in nets if m.range_check and m.fp16_mode]
    return out


def _fall_back(nets: Sequence, what: str, bits: int, probe, earlier_invalid: bool = False) -> None:
    for m in nets:  # the coarse and the fine pass run in one precision mode
        if m.fp16_mode:
            m.fall_back(what, bits, probe, earlier_invalid=earlier_invalid)
    if len({m.infer_prec() for m in nets}) > 1:  # one net could re-calibrate, another had to give up: both go to bf16x3
        for m in nets:
            if m.fp16_mode:
                m.act_scaling = False
                m.fall_back(what, bits, scaled=False)


def frame_flagged(nets: Sequence, dev, events_before: Optional[int] = None, probe=None) -> bool:
    """Deferred range check (`NeRF.range_check = "deferred"`): the one look per frame.  True when a launch of the frame
    left the fp16 envelope - the LAST one (its word is polled here) or an EARLIER chunk, which the following chunk's poll
    has consumed already (the chunk that overflowed is in the list of results all the same): any range event
    since `events_before` (the nets' summed `range_events`) says so.  The nets have been re-calibrated / switched to
    their bf16 mode (with a RuntimeWarning); the caller renders the frame again."""
    earlier = events_before is not None and sum(m.range_events for m in nets) != events_before
    if not any(m.range_check == "deferred" and m.fp16_mode for m in nets):
        return earlier
    bits = ops.range_poll(dev)
    if not bits:
        return earlier
    for m in nets:
        if m.fp16_mode:
            m.fall_back("render_frame (deferred range check at the end of the frame)", bits, probe, earlier_invalid=True)
    return True
