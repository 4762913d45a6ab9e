#!/usr/bin/env python3
"""Generate tests/golden/g7_refresh_autocast.npz by IMPORTING the reference (as make_golden.py does; nothing of it is
copied): what the reference's occupancy refresh computes for `occ_eval_fn(x) = model(x) * render_step_size` under
autocast (run-nerf.py:288-295), on fixed points and a fixed network.

    python tests/golden/make_golden_refresh.py        (build container only: needs the reference)

Contents (data only):
  x                    16,384 seeded points, uniform in the box [-1.5, 1.5]^3, float32
  sigma_weight/_bias   the sigma head used.  The network is the one of g4_nerf_8x256.npz (its `sd.*` arrays) with the
                       sigma head's weight scaled by 2048 and its bias shifted so that the 70th percentile of
                       occ = sigma * step lands on the threshold: about 30 % of the points are "occupied" and the
                       values straddle the threshold at a density that makes flipped decisions countable
  step, thre           5e-3, 1e-2
  occ_f64, occ_f32     the reference NeRF's `model(x) * step` in float64 and in float32
  occ_ac_fp16/_bf16    ... under torch.autocast("cpu", dtype=float16 / bfloat16), as float32
  dev_ref_fp16/_bf16   max |occ_ac_* - occ_f64|: the reference's own error under autocast

CPU autocast is the closest pin this build container allows for the reference's CUDA autocast (no GPU, and the GPU box
has no reference): it applies the same casting policy to the same `nn.Linear` calls (half-precision inputs and weights,
half-precision outputs), but the library behind it chooses its own accumulation order and rounding points, as the GPU
library does.  The deviations stored here are therefore a grade, not a bit pattern.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _import_reference  # noqa: E402

N, STEP, THRE, SCALE, PCT = 16384, 5e-3, 1e-2, 2048.0, 70.0


def main():
    M = _import_reference()[0]
    torch.set_num_threads(1)
    g4 = np.load(os.path.join(HERE, "g4_nerf_8x256.npz"))
    sd = {k[3:]: torch.from_numpy(g4[k]) for k in g4.files if k.startswith("sd.")}
    kw = {"pos_fn": {"n_freqs": 10, "log_space": True}, "dir_fn": {"n_freqs": 4, "log_space": True}}
    net = M.NeRF(3, 3, 8, 256, [4], **kw)
    gen = torch.Generator().manual_seed(7)
    x = torch.rand(N, 3, generator=gen) * 3.0 - 1.5
    sd["sigma.weight"] = sd["sigma.weight"] * SCALE
    net.load_state_dict(sd)
    with torch.no_grad():
        s64 = net.double()(x.double()).reshape(-1)
        # shift the bias: percentile PCT of sigma * STEP on the threshold (bias kept a float32 value)
        q = float(np.percentile(s64.numpy(), PCT))
        sd["sigma.bias"] = (sd["sigma.bias"].double() + (THRE / STEP - q)).float()
        net = M.NeRF(3, 3, 8, 256, [4], **kw)
        net.load_state_dict(sd)
        occ32 = (net(x) * STEP).reshape(-1)
        ac = {}
        for name, dt in (("fp16", torch.float16), ("bf16", torch.bfloat16)):
            with torch.autocast("cpu", dtype=dt):
                ac[name] = (net(x) * STEP).reshape(-1).float()
        occ64 = (net.double()(x.double()) * STEP).reshape(-1)
    out = {"x": x.numpy(), "sigma_weight": sd["sigma.weight"].numpy(), "sigma_bias": sd["sigma.bias"].numpy(),
           "step": np.array(STEP), "thre": np.array(THRE), "occ_f64": occ64.numpy(), "occ_f32": occ32.numpy()}
    for name, v in ac.items():
        out["occ_ac_" + name] = v.numpy()
        out["dev_ref_" + name] = np.array(float((v.double() - occ64).abs().max()))
    np.savez_compressed(os.path.join(HERE, "g7_refresh_autocast.npz"), **out)
    on = occ64.numpy() > THRE
    print(f"occ {occ64.min():.3f} .. {occ64.max():.3f}, {100 * on.mean():.1f} % above the threshold, finite: "
          f"{bool(np.isfinite(occ64.numpy()).all())}, float32 dev {float((occ32.double() - occ64).abs().max()):.2e}")
    for name, v in ac.items():
        dev = float(out["dev_ref_" + name])
        flips = (v.numpy() > THRE) != on
        band = np.abs(occ64.numpy() - THRE) <= 2 * dev
        print(f"{name}: dev_ref {dev:.2e}, {int(flips.sum())} flipped decisions ({int((flips & ~band).sum())} outside 2 x dev_ref), "
              f"{100 * band.mean():.2f} % of the points inside the band")


if __name__ == "__main__":
    main()
