"""The premise of tests/test_two_pass_gpu.py, on the CPU.  precision="fp16x2" forms ah.wh + 2^-11 al'.wh per GEMM
(the FSN_PREC_FP16X3 blob with the weights' low fragments unread); fp16x3 without activation scaling forms
ah.wh + 2^-11 (al'.wh + ah.wl').  With every split GEMM weight exactly representable in fp16, wl' = 0 and the two form
the same sums.  R(W) is W with those weights rounded: layers.*.weight, connection.weight and branch.weight - the
GEMMs of gemm_to_sd / pack_piece (csrc/mlp_pack.hpp), which packs half_rne(w) and half_rne((w - hi) 2^11); biases,
sigma.* and rgb.* are aux_value's float32 entries and stay as they are.

Also here: 8x256 with skip (4,) reaches every hand-scheduled k-loop block shape of tools/gen_kloop.py, so the GPU
file's runs on it execute all nine, in every parity a network can reach them in (ten of the generator's eighteen
texts per mode: test_8x256_reaches_every_hand_scheduled_block).
"""
import functools
import importlib.util
import os

import torch

import wstream_ref as W
from oracle import fsnerf_oracle as O

N = 300
NET = (4, 128, (4,), 10, 4)
CFG = dict(n_layers=4, skip=[4], n_freqs=10, n_freqs_dir=4, log_space=True)
SPLIT_GEMMS = ("layers.", "connection.", "branch.")


def rounded(sd):
    """R(W): the weights the packer splits into fp16 high and low parts, rounded to fp16."""
    return {k: (v.half().to(v.dtype) if k.endswith(".weight") and k.startswith(SPLIT_GEMMS) else v.clone())
            for k, v in sd.items()}


def gemm_names(n_layers):
    """Kernel GEMM order: hidden 0 .. L-1, connection, branch."""
    return [f"layers.{i}.weight" for i in range(n_layers)] + ["connection.weight", "branch.weight"]


def scaled(sd, n_layers, exps):
    """The split GEMMs' weights x 2^exps[g] (kernel GEMM order), everything else as it is."""
    out = dict(sd)
    for g, k in enumerate(gemm_names(n_layers)):
        out[k] = sd[k] * 2.0 ** exps[g]
    return out


# tests/test_two_pass_gpu.py (a): the 8x256 network with its split weights scaled by exact powers of two
POW2 = {"all-down": [-7] * 10, "even-up": [7 if g % 2 == 0 else -7 for g in range(10)],
        "odd-up": [-7 if g % 2 == 0 else 7 for g in range(10)]}


@functools.lru_cache(maxsize=None)
def setup():
    L, D, skip, nf, nfd = NET
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=7)
    gen = torch.Generator().manual_seed(20)
    x = torch.rand(N, 3, generator=gen) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    return sd, x, d


def test_rounding_touches_the_split_gemms_only():
    sd, _, _ = setup()
    r = rounded(sd)
    changed = {k for k in sd if not torch.equal(sd[k], r[k])}
    assert changed == {f"layers.{i}.weight" for i in range(4)} | {"connection.weight", "branch.weight"}
    for k in changed:
        assert torch.equal(r[k], r[k].half().float()) and float((r[k] - sd[k]).abs().max()) <= 2.0 ** -11 * float(sd[k].abs().max())


def test_x2_emulation_is_the_x3_emulation_on_fp16_weights():
    sd, x, d = setup()
    for dt in (torch.float32, torch.float64):
        w = {k: v.to(dt) for k, v in sd.items()}
        r = rounded(w)
        for dirs in (d.to(dt), None):
            a = O.nerf_forward(w, x.to(dt), dirs, emulate="fp16x2", **CFG)
            b = O.nerf_forward(r, x.to(dt), dirs, emulate="fp16x3", **CFG)
            assert a.dtype == dt and bool(torch.isfinite(a).all())
            assert torch.equal(a, b), f"{dt}: differs by up to {float((a - b).abs().max()):.3e}"
        # not vacuous: on the natural weights the weights' low parts matter
        assert not torch.equal(O.nerf_forward(w, x.to(dt), d.to(dt), emulate="fp16x2", **CFG),
                               O.nerf_forward(w, x.to(dt), d.to(dt), emulate="fp16x3", **CFG))


def test_x2_emulation_is_float32_grade_on_the_rounded_weights():
    """The bars of tests/test_shape_corners_gpu.py for the x3 arithmetic: rgb 1e-5, sigma 1e-4 max|sigma| (+ rtol 1e-4)."""
    sd, x, d = setup()
    w = {k: v.double() for k, v in sd.items()}
    y = O.nerf_forward(w, x.double(), d.double(), emulate="fp16x2", **CFG)
    want = O.nerf_forward(rounded(w), x.double(), d.double(), **CFG)
    smax = float(want[:, 3].abs().max())
    e_rgb, e_sigma = float((y[:, :3] - want[:, :3]).abs().max()), float((y[:, 3] - want[:, 3]).abs().max()) / smax
    print(f"x2 emulation against float64 on R(W): rgb {e_rgb:.2e}, sigma/max {e_sigma:.2e}")
    assert bool(((y[:, :3] - want[:, :3]).abs() <= 1e-5 + 1e-4 * want[:, :3].abs()).all())
    assert bool(((y[:, 3] - want[:, 3]).abs() <= 1e-4 * smax + 1e-4 * want[:, 3].abs()).all())


def test_8x256_reaches_every_hand_scheduled_block():
    """The block shapes gemm_layer asks for on 8x256 / skip (4,) are exactly the generator's nine; a network without a
    reachable skip (`wide-min`) has no 20-unit pair."""
    spec = importlib.util.spec_from_file_location(
        "gen_kloop", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "gen_kloop.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    L, D, skip = 8, 256, (4,)
    assert sum(2 * npo * ks for npo, ks in W.gemms(L, D, skip)) == W.units(L, D, 1)[1]
    assert sum(2 * npo * ks for npo, ks in W.gemms(L, D, skip)[:L]) == W.units(L, D, 1)[0]
    shapes = W.kloop_shapes(L, D, skip)
    assert shapes == set(gen.SHAPES) == {(16, 0), (20, 0), (20, 4), (18, 0), (18, 2), (18, 4), (18, 6), (4, 0), (4, 4)}
    # with the parity (PAR = tp & 1): an offset other than 0 mod 8 fixes the parity of tp, so of the generator's 18
    # texts per mode these ten are the ones any network can instantiate, and 8x256 / (4,) instantiates them all
    texts = {(2 * ks, (tp * 2 * ks) % 8, tp & 1) for npo, ks in W.gemms(L, D, skip) for tp in range(npo)}
    assert texts == {(16, 0, 0), (16, 0, 1), (20, 0, 0), (20, 4, 1), (18, 0, 0), (18, 2, 1), (18, 4, 0), (18, 6, 1),
                     (4, 0, 0), (4, 4, 1)}
    assert (20, 0) not in W.kloop_shapes(*W.CORNERS["wide-min"][:3])
    for net in ("wide-skips", "wide-min"):
        Lc, Dc, sc = W.CORNERS[net][:3]
        assert W.kloop_shapes(Lc, Dc, sc) <= shapes
        assert sum(2 * npo * ks for npo, ks in W.gemms(Lc, Dc, sc)) == W.units(Lc, Dc, len(sc))[1]


def test_power_of_two_networks_and_why_none_is_all_up():
    """Every split weight x 2^7 leaves the fp16 range in exact arithmetic (the activations grow ~50 x per layer), so no
    fp16 mode can run it without a range flag; POW2's three networks stay well inside the envelope and every GEMM has
    its weights at 2^7 in one of them."""
    L, D, skip, nf, nfd = 8, 256, (4,), 10, 4
    cfg = dict(n_layers=L, skip=list(skip), n_freqs=nf, n_freqs_dir=nfd)
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=7)
    _, x, d = setup()
    up = O.layer_maxima(rounded(scaled(sd, L, [7] * 10)), x, d, **cfg)
    assert up[1] < 65504.0 < up[2] and up[-1] > 1e17, up
    for case, exps in POW2.items():
        mx = O.layer_maxima(rounded(scaled(sd, L, exps)), x, d, **cfg)
        print(case, [f"{v:.3g}" for v in mx])
        assert 2.0 ** -6 < min(mx) and max(mx) < 65504.0 / 64, (case, mx)
    assert all(any(POW2[c][g] == 7 for c in POW2) and any(POW2[c][g] == -7 for c in POW2) for g in range(10))
