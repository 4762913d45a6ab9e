"""LPIPS-VGG as a loss, restated on the CPU from the algorithm: the value of tests/lpips_ref.py and the gradient of
sum_n up[n] * lpips_n with respect to the two images, written out layer by layer (no autograd) in float64 (the truth) or
float32 (the yardstick for float32 arithmetic), with the two definitions the kernels use where autograd has none or
leaves a choice:
  * a pixel whose tap vector is all zero gets gradient 0 from the head (autograd: NaN, 0 * inf from sqrt);
  * a pooled gradient goes to the FIRST maximum of its 2 x 2 window in row-major order (max_pool2d's rule); sizes
    floor, so an odd last row or column lies in no window.
Also `margins`, which says how far a forward is from flipping a ReLU unit or a pool winner, the committed GPU test
cases (seeds for which no float32 forward can flip one), and the search that found them."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lpips_ref as LR  # noqa: E402

EPS = LR.EPS
N_LAYERS = len(LR.CONVS)
TAP_OF = [LR.TAP_AFTER.get(i, -1) for _, i, _, _ in LR.CONVS]  # layer -> tap, or -1
POOL_IN = [i in LR.POOL_BEFORE for _, i, _, _ in LR.CONVS]


def _wb(sd, l, dtype):
    s, i, _, _ = LR.CONVS[l]
    return sd[f"net.slice{s}.{i}.weight"].to(dtype), sd[f"net.slice{s}.{i}.bias"].to(dtype)


def _scaling(sd, dtype):
    shift = sd.get("scaling_layer.shift", torch.tensor(LR.SHIFT)).to(dtype).reshape(1, 3, 1, 1)
    scale = sd.get("scaling_layer.scale", torch.tensor(LR.SCALE)).to(dtype).reshape(1, 3, 1, 1)
    return shift, scale


def _windows(t):
    """The four candidates of every 2 x 2 window in row-major order: [4, N, C, H // 2, W // 2]."""
    Hp, Wp = t.shape[2] // 2, t.shape[3] // 2
    t = t[:, :, :2 * Hp, :2 * Wp]
    return torch.stack([t[:, :, 0::2, 0::2], t[:, :, 0::2, 1::2], t[:, :, 1::2, 0::2], t[:, :, 1::2, 1::2]])


def _first_max(v):
    """v: [4, ...] -> boolean [4, ...], True at the first maximum of each window."""
    win = torch.zeros_like(v, dtype=torch.bool)
    taken = torch.zeros_like(v[0], dtype=torch.bool)
    top = v.max(dim=0).values
    for r in range(4):
        win[r] = (v[r] == top) & ~taken
        taken |= win[r]
    return win


def forward(sd, x, normalize=False, dtype=torch.float64):
    """x: (N, 3, H, W) -> (pre, act): the 13 pre-activations and post-ReLU activations, in `dtype`."""
    shift, scale = _scaling(sd, dtype)
    t = x.to(dtype)
    if normalize:
        t = 2 * t - 1
    t = (t - shift) / scale
    pre, act = [], []
    for l in range(N_LAYERS):
        if POOL_IN[l]:
            t = _windows(t).max(dim=0).values
        w, b = _wb(sd, l, dtype)
        p = F.conv2d(t, w, b, padding=1)
        t = p.clamp_min(0)
        pre.append(p)
        act.append(t)
    return pre, act


def value_and_grad(sd, x, y, up=None, normalize=False, dtype=torch.float64, taps=(0, 1, 2, 3, 4)):
    """-> (value [N], per-layer [5, N], dx, dy): LPIPS of the N pairs and the gradient of sum_n up[n] * value[n]
    (up: N values, default ones) with respect to x and y, (N, 3, H, W), all in `dtype`.  `taps`: the head terms that
    enter the gradient (all five: the loss's; one: that tap's share)."""
    with torch.no_grad():
        N = x.shape[0]
        up = torch.ones(N, dtype=dtype) if up is None else up.to(dtype).reshape(N)
        _, ax = forward(sd, x, normalize, dtype)
        _, ay = forward(sd, y, normalize, dtype)
        per, head_x, head_y = [], {}, {}
        for l in range(N_LAYERS):
            t = TAP_OF[l]
            if t < 0:
                continue
            fx, fy = ax[l], ay[l]
            lin = sd[f"lin{t}.model.1.weight"].to(dtype).reshape(1, -1, 1, 1)
            sx = torch.sqrt((fx * fx).sum(dim=1, keepdim=True))
            sy = torch.sqrt((fy * fy).sum(dim=1, keepdim=True))
            ux, uy = fx / (sx + EPS), fy / (sy + EPS)
            d = ux - uy
            per.append((lin * d * d).sum(dim=1).mean(dim=(1, 2)))
            HW = fx.shape[2] * fx.shape[3]
            g = 2 * lin * d * (up.reshape(N, 1, 1, 1) / HW)
            if t not in taps:
                g = torch.zeros_like(g)

            def through_norm(gg, f, s):
                nz = s > 0
                s1 = torch.where(nz, s, torch.ones_like(s))
                out = gg / (s1 + EPS) - f * (gg * f).sum(dim=1, keepdim=True) / (s1 * (s1 + EPS) ** 2)
                return torch.where(nz, out, torch.zeros_like(out))  # the all-zero pixel: 0

            head_x[l], head_y[l] = through_norm(g, fx, sx), through_norm(-g, fy, sy)
        per = torch.stack(per)
        shift, scale = _scaling(sd, dtype)

        def backward(act, head):
            G = None  # gradient w.r.t. the layer's pre-activation
            for l in range(N_LAYERS - 1, -1, -1):
                a = act[l]
                if TAP_OF[l] >= 0:
                    tot = head[l].clone()
                    if G is not None:  # G: w.r.t. the pooled tap, the input of layer l + 1
                        Hp, Wp = G.shape[2], G.shape[3]
                        win = _first_max(_windows(a))
                        for r, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                            tot[:, :, i:2 * Hp:2, j:2 * Wp:2] += torch.where(win[r], G, torch.zeros_like(G))
                    G = torch.where(a > 0, tot, torch.zeros_like(tot))
                else:
                    G = torch.where(a > 0, G, torch.zeros_like(G))
                # data gradient of layer l: conv3x3(G, W') with W'[ci][co][tap] = W[co][ci][8 - tap]
                w, _ = _wb(sd, l, dtype)
                G = F.conv2d(G, w.transpose(0, 1).flip(2, 3), padding=1)
            G = G / scale
            return 2 * G if normalize else G

        return per.sum(dim=0), per, backward(ax, head_x), backward(ay, head_y)


def autograd_value_and_grad(sd, x, y, up=None, normalize=False, dtype=torch.float64):
    """lpips_ref's formula re-run with torch autograd: (value [N], dx, dy).  NaN at an all-zero tap pixel."""
    shift, scale = _scaling(sd, dtype)
    x = x.to(dtype).clone().requires_grad_(True)
    y = y.to(dtype).clone().requires_grad_(True)

    def features(t):
        if normalize:
            t = 2 * t - 1
        t = (t - shift) / scale
        taps = []
        for l in range(N_LAYERS):
            if POOL_IN[l]:
                t = F.max_pool2d(t, 2, 2)
            w, b = _wb(sd, l, dtype)
            t = F.relu(F.conv2d(t, w, b, padding=1))
            if TAP_OF[l] >= 0:
                taps.append(t)
        return taps

    total = 0
    for k, (a, b) in enumerate(zip(features(x), features(y))):
        na = a / (torch.sqrt(torch.sum(a * a, dim=1, keepdim=True)) + EPS)
        nb = b / (torch.sqrt(torch.sum(b * b, dim=1, keepdim=True)) + EPS)
        lin = F.conv2d((na - nb) ** 2, sd[f"lin{k}.model.1.weight"].to(dtype))
        total = total + lin.mean(dim=(1, 2, 3))
    up = torch.ones_like(total) if up is None else up.to(dtype)
    (total * up).sum().backward()
    return total.detach(), x.grad, y.grad


def margins(sd, x, y, normalize=False):
    """Per layer (13 rows): [the smallest |pre-activation| of the float64 forward over both images; the smallest gap
    between the winner and the runner-up over the pool windows whose maximum is positive (inf for a layer no pool
    follows); the largest |float32 - float64| pre-activation difference].  A float32 forward whose error stays a
    safe factor below the first two cannot flip a ReLU unit or a pool winner."""
    rows = []
    with torch.no_grad():
        p64 = [forward(sd, t, normalize, torch.float64) for t in (x, y)]
        p32 = [forward(sd, t, normalize, torch.float32) for t in (x, y)]
        for l in range(N_LAYERS):
            small = min(float(p[0][l].abs().min()) for p in p64)
            gap = float("inf")
            if l + 1 < N_LAYERS and POOL_IN[l + 1]:
                for p in p64:
                    v = _windows(p[1][l]).sort(dim=0, descending=True).values
                    pos = v[0] > 0
                    if bool(pos.any()):
                        gap = min(gap, float((v[0] - v[1])[pos].min()))
            diff = max(float((a[0][l].double() - b[0][l]).abs().max()) for a, b in zip(p32, p64))
            rows.append((small, gap, diff))
    return rows


SAFETY = 16.0  # every margin at least this many float32-vs-float64 differences
# Where no seed reaches SAFETY: the accuracy bar grants float32 arithmetic four times the float32 restatement's error
# (E(hip) <= 4 E(f32) + 1e-6), so a forward inside that allowance cannot flip a unit whose margin is four differences.
SAFETY_LARGE = 4.0


def safety_of(rows):
    """The smallest margin in units of its layer's float32-vs-float64 difference."""
    return min(min(small, gap) / diff for small, gap, diff in rows)


def make_pair(seed, N, H, W):
    """Two batches of N uniform random images in [0, 1], float32 (N, 3, H, W)."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(N, 3, H, W, generator=g), torch.rand(N, 3, H, W, generator=g)


SD_SEED = 7  # lpips_ref.random_state_dict(seed=SD_SEED)

# name -> (H, W, seeds, normalize, factor): pair n of the GPU test's inputs is make_pair(seeds[n], 1, H, W) (2v - 1 of it
# when normalize is False), and every layer's smallest margin is at least `factor` float32-vs-float64 differences
# (tests/test_lpips_grad_cpu.py asserts it).  The number of units within reach of a flip grows with the pixel count:
# at 16 x 16 seed 12 is the first of 13 that reaches SAFETY; at 37 x 53 the best of seeds 0..1838 reaches 4.6 and at
# 32 x 32 the best three of seeds 0..1297 reach 6.4, 6.3 and 5.4 (about forty units of a 37 x 53 pair lie within 16
# differences of zero whatever the seed), so those cases carry the best seeds found and SAFETY_LARGE.  `best_seeds`
# below is the search.
CASES = {
    "16x16": (16, 16, (12,), False, SAFETY),   # stage 5 is one pixel, the tiles mostly empty
    "16x16n": (16, 16, (12,), True, SAFETY),
    "37x53": (37, 53, (1444,), True, SAFETY_LARGE),  # odd through every pool; the last row and column in no window
    "32x32x3": (32, 32, (323, 469, 75), False, SAFETY_LARGE),  # the batched z index
}


def case_inputs(name):
    H, W, seeds, normalize, _ = CASES[name]
    pairs = [make_pair(seed, 1, H, W) for seed in seeds]
    x, y = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    if not normalize:
        x, y = 2 * x - 1, 2 * y - 1
    return x, y, normalize


def best_seeds(H, W, normalize, seeds=range(0, 2000), keep=3, enough=SAFETY):
    """[(safety, seed)] of the `keep` best single pairs among `seeds`; stops at the first that reaches `enough`."""
    sd = LR.random_state_dict(SD_SEED)
    found = []
    for seed in seeds:
        x, y = make_pair(seed, 1, H, W)
        if not normalize:
            x, y = 2 * x - 1, 2 * y - 1
        found.append((safety_of(margins(sd, x, y, normalize)), seed))
        if found[-1][0] >= enough:
            break
    return sorted(found, reverse=True)[:keep]


if __name__ == "__main__":  # python tests/lpips_grad_ref.py H W normalize [seeds]
    a = sys.argv[1:]
    print(best_seeds(int(a[0]), int(a[1]), bool(int(a[2])), range(int(a[3]) if len(a) > 3 else 2000)))
