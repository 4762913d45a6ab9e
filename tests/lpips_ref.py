"""LPIPS v0.1 with the VGG16 backbone, restated in torch on the CPU from the algorithm (no `lpips` package needed), in
float64 (the truth) or float32 (the yardstick for float32 arithmetic).  It reads the `lpips` package's state-dict keys:
scaling_layer.shift / scale (optional: the package's constants), net.sliceK.I.weight / bias at torchvision's `features`
indices, linK.model.1.weight.  Also: a seeded random state dict in that layout, for tests."""
import math

import torch
import torch.nn.functional as F

# (slice, features index, Cin, Cout) of the 13 convolutions; a 2x2 max-pool precedes the first conv of slices 2..5
CONVS = ((1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256),
         (3, 14, 256, 256), (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512),
         (5, 26, 512, 512), (5, 28, 512, 512))
TAP_AFTER = {2: 0, 7: 1, 14: 2, 21: 3, 28: 4}  # features index of relu1_2 ... relu5_3's conv -> tap
POOL_BEFORE = {5, 10, 17, 24}
TAP_CHANNELS = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10


def state_dict_shapes():
    """key -> shape of the package's LPIPS(net="vgg") state dict (without the `lins.*` aliases)."""
    out = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    for s, i, cin, cout in CONVS:
        out[f"net.slice{s}.{i}.weight"] = (cout, cin, 3, 3)
        out[f"net.slice{s}.{i}.bias"] = (cout,)
    for k, c in enumerate(TAP_CHANNELS):
        out[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return out


def random_state_dict(seed: int = 0):
    """He-normal convolutions, small random biases, non-negative lin weights (as trained heads are), float32."""
    g = torch.Generator().manual_seed(seed)
    sd = {"scaling_layer.shift": torch.tensor(SHIFT)[None, :, None, None],
          "scaling_layer.scale": torch.tensor(SCALE)[None, :, None, None]}
    for s, i, cin, cout in CONVS:
        sd[f"net.slice{s}.{i}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        sd[f"net.slice{s}.{i}.bias"] = 0.02 * (torch.rand(cout, generator=g) - 0.5)
    for k, c in enumerate(TAP_CHANNELS):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    return sd


def lpips(sd, x, y, normalize=False, dtype=torch.float64):
    """x, y: (N, 3, H, W) CPU tensors.  Returns (value [N], per-layer [5, N]) in `dtype`: the five taps' spatial means
    of sum_c lin_c (f_x / (|f_x| + eps) - f_y / (|f_y| + eps))^2, and their sum."""
    shift = sd.get("scaling_layer.shift", torch.tensor(SHIFT)[None, :, None, None]).to(dtype).reshape(1, 3, 1, 1)
    scale = sd.get("scaling_layer.scale", torch.tensor(SCALE)[None, :, None, None]).to(dtype).reshape(1, 3, 1, 1)

    def features(t):
        t = t.to(dtype)
        if normalize:
            t = 2 * t - 1
        t = (t - shift) / scale
        taps = []
        for s, i, _, _ in CONVS:
            if i in POOL_BEFORE:
                t = F.max_pool2d(t, 2, 2)
            t = F.relu(F.conv2d(t, sd[f"net.slice{s}.{i}.weight"].to(dtype), sd[f"net.slice{s}.{i}.bias"].to(dtype),
                                padding=1))
            if i in TAP_AFTER:
                taps.append(t)
        return taps

    with torch.no_grad():
        fx, fy = features(x), features(y)
        per = []
        for k, (a, b) in enumerate(zip(fx, fy)):
            na = a / (torch.sqrt(torch.sum(a * a, dim=1, keepdim=True)) + EPS)
            nb = b / (torch.sqrt(torch.sum(b * b, dim=1, keepdim=True)) + EPS)
            d = (na - nb) ** 2
            lin = F.conv2d(d, sd[f"lin{k}.model.1.weight"].to(dtype))
            per.append(lin.mean(dim=(1, 2, 3)))
        per = torch.stack(per)
        return per.sum(dim=0), per
