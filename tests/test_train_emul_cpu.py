"""The restatement of the single-pass training step (tests/train_emul_ref.py) checked without a GPU, and the yardsticks
the GPU test (tests/test_single_pass_grad_gpu.py) holds the kernels to: `pinned` / `natural` build a case once per
process - inputs, cotangent, network, float64 autograd's gradients, the restatement's gradients and the restatement's
own error per tensor - and the GPU test imports them.

The pinned networks are the GPU test's premise: a network where no ReLU unit can change branch under the mode's forward
error.  The conditions are asserted here, for every network, mode and input form the GPU test runs, so that it cannot
lose its premise silently.

The restatement's own errors are bounded here as well (`error_cap`), because the GPU test's bar is a multiple of them: a
restatement that is wrong about a tensor would otherwise widen that tensor's bar."""
import functools

import pytest
import torch

import train_emul_ref as R
from oracle import fsnerf_oracle as O

# The training envelope's own corners (tests/test_train_step.py, tests/test_shape_corners_gpu.py)
NETS = {"8x256": (8, 256, (4,), 10, 4), "6x128": (6, 128, (1, 3), 7, 3), "2x128": (2, 128, (), 10, 4)}
MODES = ("fp16", "bf16")
N = 300        # two full 128-sample tiles and a ragged one
N_RAYS = 7
N_NATURAL = 777
RAY_NET = "6x128"
CSCALES = (1e-7, 1e3)  # fp16, 6x128: cotangent sizes beside 1.0, for the gradient scaling
UNIT = {"fp16": 2.0 ** -11, "bf16": 2.0 ** -8}  # unit roundoff of the formats


def error_cap(net, mode):
    """Upper bound on the restatement's error in any gradient tensor, relative to the tensor's largest entry: a gradient
    entry is a sum of products whose factors went through at most n_layers + 3 GEMMs of the chain (forward or backward),
    each of which rounds both operands: 2 (n_layers + 3) roundings of relative size u, added linearly (no cancellation
    assumed between them, none of the growth a sum over samples with mixed signs can add: the pinned networks measure
    0.1 .. 0.4 of this)."""
    return 2.0 * (NETS[net][0] + 3) * UNIT[mode]


@functools.lru_cache(maxsize=None)
def pinned_inputs(form):
    """300 points in the box and 300 packed intervals on 7 rays (the samples of tests/test_shape_corners_gpu.py), and one
    cotangent."""
    gen = torch.Generator().manual_seed(20)
    x = torch.rand(N, 3, generator=gen) * 3 - 1.5
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=gen), dim=-1)
    o = torch.rand(N_RAYS, 3, generator=gen) - 0.5
    rd = torch.nn.functional.normalize(torch.randn(N_RAYS, 3, generator=gen), dim=-1)
    ri = (torch.arange(N) * N_RAYS) // N
    t0 = 0.5 + torch.rand(N, generator=gen) * 2.0
    t1 = t0 + 0.01 + torch.rand(N, generator=gen) * 0.05
    c = torch.randn(N, 4, generator=gen)
    if form == "rays":
        return {"o": o, "d": rd, "ri": ri, "t0": t0, "t1": t1}, c
    return {"x": x, "d": d}, c


def samples_of(inputs):
    """(x, d) float64 of either input form."""
    if "ri" in inputs:
        ri = inputs["ri"]
        mid = ((inputs["t0"].double() + inputs["t1"].double()) / 2.0)[:, None]
        return inputs["o"].double()[ri] + inputs["d"].double()[ri] * mid, inputs["d"].double()[ri]
    return inputs["x"].double(), inputs["d"].double()


@functools.lru_cache(maxsize=None)
def pinned_network(net, form):
    x, d = samples_of(pinned_inputs(form)[0])
    return R.pinned_state_dict(NETS[net], x, d, seed=7)


@functools.lru_cache(maxsize=None)
def pinned(net, mode, form="point", cscale=1.0):
    """One pinned case: dict(inputs, c, sd, scale, want, emul, yard).  want / emul: gradients of (out * c).sum() by float64
    autograd / by the restatement in `mode`; yard = R.entry_metrics(emul, want): the restatement's own errors.  Raises
    where one of them exceeds error_cap: the yardstick itself is then wrong."""
    inputs, c = pinned_inputs(form)
    c = c * cscale
    sd = pinned_network(net, form)
    scale = R.grad_scale(c) if mode == "fp16" else 1.0
    _, want = R.gradients(sd, inputs, c, NETS[net], None)
    _, emul = R.gradients(sd, inputs, c, NETS[net], mode, scale)
    yard = R.entry_metrics(emul, want, NETS[net])
    cap = error_cap(net, mode)
    over = {k: v for k, v in yard.items() if not v <= cap}
    assert not over, f"{net} {mode} {form} x{cscale:g}: the restatement's own error exceeds {cap:.2e}: {over}"
    return dict(inputs=inputs, c=c, sd=sd, scale=scale, want=want, emul=emul, yard=yard)


@functools.lru_cache(maxsize=None)
def natural_inputs():
    gen = torch.Generator().manual_seed(0)
    x = torch.rand(N_NATURAL, 3, generator=gen) * 2 - 1
    d = torch.nn.functional.normalize(torch.randn(N_NATURAL, 3, generator=gen), dim=-1)
    c = torch.randn(N_NATURAL, 4, generator=gen)
    return {"x": x, "d": d}, c


@functools.lru_cache(maxsize=None)
def natural_network(net):
    """The initialisation of tests/test_train_step.py::test_nerf_gradients_vs_autograd."""
    L, D, skip, nf, nfd = NETS[net]
    sd = O.init_nerf_state_dict(L, D, list(skip), nf, nfd, seed=3)
    sd["sigma.weight"] = sd["sigma.weight"] * 16.0
    return sd


@functools.lru_cache(maxsize=None)
def natural(net, mode):
    """One natural case (ReLU masks differ from sample to sample, units near zero change branch under the mode's error):
    dict(inputs, c, sd, scale, want, emul, yard) with yard = R.l2_metrics(emul, want)."""
    inputs, c = natural_inputs()
    sd = natural_network(net)
    scale = R.grad_scale(c) if mode == "fp16" else 1.0
    _, want = R.gradients(sd, inputs, c, NETS[net], None)
    _, emul = R.gradients(sd, inputs, c, NETS[net], mode, scale)
    return dict(inputs=inputs, c=c, sd=sd, scale=scale, want=want, emul=emul, yard=R.l2_metrics(emul, want, NETS[net]))


# the (network, mode, form, cotangent scale) of every pinned case the GPU test runs
PINNED_CASES = [(net, mode, "point", 1.0) for net in NETS for mode in MODES] + \
               [(RAY_NET, mode, "rays", 1.0) for mode in MODES] + [(RAY_NET, "fp16", "point", s) for s in CSCALES]


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("net", list(NETS))
def test_without_rounding_the_restatement_is_float64_autograd(net):
    """fmt=None: output and every gradient equal float64 autograd on O.nerf_forward to 1e-12 (natural network: masks
    differ from sample to sample), point form and, on one network, ray form."""
    forms = [natural_inputs()] + ([pinned_inputs("rays")] if net == RAY_NET else [])
    for inputs, c in forms:
        sd = natural_network(net)
        out, got = R.gradients(sd, inputs, c, NETS[net], None)
        par = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
        if "ri" in inputs:
            a, b = inputs["o"].double().requires_grad_(True), inputs["d"].double().requires_grad_(True)
            mid = ((inputs["t0"].double() + inputs["t1"].double()) / 2.0)[:, None]
            x, d = a[inputs["ri"]] + b[inputs["ri"]] * mid, b[inputs["ri"]]
            names = ("d_rays_o", "d_rays_d")
        else:
            a, b = inputs["x"].double().requires_grad_(True), inputs["d"].double().requires_grad_(True)
            x, d = a, b
            names = ("d_x", "d_dirs")
        ref = O.nerf_forward(par, x, d, **R.cfg_of(NETS[net]))
        (ref * c.double()).sum().backward()
        want = {k: v.grad for k, v in par.items()}
        want[names[0]], want[names[1]] = a.grad, b.grad
        assert set(got) == set(want)
        assert R.rel_max(out, ref) <= 1e-12
        for k in want:
            assert R.rel_max(got[k], want[k]) <= 1e-12, (k, R.rel_max(got[k], want[k]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("net", list(NETS))
def test_the_restatements_forward_is_the_oracles_emulation_bit_for_bit(net, mode):
    for sd, (inputs, _) in ((natural_network(net), natural_inputs()), (pinned_network(net, "point"), pinned_inputs("point"))):
        x, d = samples_of(inputs)
        with torch.no_grad():
            got = R.forward(sd, x, d, NETS[net], mode)
            want = O.nerf_forward({k: v.double() for k, v in sd.items()}, x, d, emulate=mode, **R.cfg_of(NETS[net]))
        assert got.dtype == torch.float64 and torch.equal(got, want)


def test_the_gradient_scale_is_the_kernels_rule():
    """fsn_grad_scale: 2^clamp(floor(log2(1024 / max)), -40, 60), 1 for 0 / inf / NaN."""
    t = lambda *v: torch.tensor(v)
    assert R.grad_scale(t(1.0, -3.0)) == 256.0          # 1024 / 3 = 341.3
    assert R.grad_scale(t(1024.0)) == 1.0 and R.grad_scale(t(1025.0)) == 0.5
    assert R.grad_scale(t(1e-30)) == 2.0 ** 60 and R.grad_scale(t(1e30)) == 2.0 ** -40
    assert R.grad_scale(t(0.0)) == 1.0 and R.grad_scale(t(float("inf"))) == 1.0 and R.grad_scale(t(float("nan"))) == 1.0


# ------------------------------------------------------------------------------------------------ the pinned networks
@pytest.mark.parametrize("net,mode,form,cscale", PINNED_CASES)
def test_pinned_network_conditions(net, mode, form, cscale):
    """The GPU test's premise, per case: every ReLU pre-activation is at least 0.5 from zero in float64 (and at most 1.5),
    each unit has one sign over all samples, the restatement moves no pre-activation by more than 0.01 and flips none."""
    sd = pinned_network(net, form)
    x, d = samples_of(pinned_inputs(form)[0])
    z = R.preacts(sd, x, d, NETS[net])
    ze = R.preacts(sd, x, d, NETS[net], mode)
    L, D = NETS[net][:2]
    assert z.shape == (N, L * D + D // 2)
    lo, hi, err = float(z.abs().min()), float(z.abs().max()), float((ze - z).abs().max())
    on = (z > 0).sum(0)
    share = float((on == N).float().mean())
    print(f"{net} {mode} {form}: |z| in [{lo:.6f}, {hi:.6f}], {share:.2f} of the units on, restatement moves z by {err:.2e}")
    assert lo >= 0.5 and hi <= 1.5
    assert bool(((on == 0) | (on == N)).all()), "a unit is on for some samples and off for others"
    assert 0.3 < share < 0.7
    assert err <= 0.01
    assert int(((ze > 0) != (z > 0)).sum()) == 0
    assert all(v.dtype == torch.float32 for v in sd.values())


@pytest.mark.parametrize("net,mode,form,cscale", PINNED_CASES)
def test_pinned_yardstick(net, mode, form, cscale):
    """The restatement's own per-tensor error against float64 on the pinned networks (the GPU test's bar is 4 x these):
    finite, below error_cap (asserted by `pinned` itself), non-zero where operands are rounded; the head biases, which no
    rounded operand enters but through the forward's rgb, within the fp32-grade floor of 2e-4."""
    case = pinned(net, mode, form, cscale)
    yard, want = case["yard"], case["want"]
    whole = {k: v for k, v in yard.items() if "[" not in k}
    inp = ("d_rays_o", "d_rays_d") if form == "rays" else ("d_x", "d_dirs")
    assert set(whole) == set(case["sd"]) | set(inp)
    for k, v in sorted(whole.items()):
        print(f"{net} {mode} {form} x{cscale:g} {k}: restatement {v:.2e}, largest entry {float(want[k].abs().max()):.2e}")
    assert all(float(want[k].abs().max()) > 0 for k in whole)
    assert all(0 <= v <= error_cap(net, mode) for v in yard.values())
    assert yard["sigma.bias"] <= 2e-4 and yard["rgb.bias"] <= 2e-4
    for k, v in whole.items():
        if k not in ("sigma.bias", "rgb.bias"):
            assert v > 0.02 * UNIT[mode], (k, v)
    for k, blocks in R.column_splits(NETS[net]).items():
        assert all(f"{k}[{lab}]" in yard for lab, _ in blocks)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("net", list(NETS))
def test_natural_yardstick(net, mode):
    """The natural networks: the restatement's relative L2 error per tensor is finite and, but for the head biases,
    non-zero - units do change branch there, which is why these bars are statistical."""
    case = natural(net, mode)
    for k, (err, n_got, n_want, finite) in sorted(case["yard"].items()):
        if "[rows" not in k:
            print(f"{net} {mode} {k}: restatement L2 {err:.2e}")
            assert finite and n_want > 0 and err < 0.5, (k, err)
            assert err > 0 or k in ("sigma.bias", "rgb.bias"), k  # (sigma.bias: the sum of the cotangent's last column)


def test_metrics_see_a_dropped_bias_a_zeroed_row_block_and_swapped_column_blocks():
    """The three faults the whole-gradient cosine tests pass, applied to float64's own gradients: each must exceed the
    bar max(4 x yardstick, 2e-4) under R.entry_metrics, in the key that names it."""
    net, mode = "6x128", "bf16"
    case = pinned(net, mode)
    want, yard = case["want"], case["yard"]
    D = NETS[net][1]

    def failing(got):
        m = R.entry_metrics(got, want, NETS[net])
        return {k for k, v in m.items() if v > max(4.0 * yard[R.base_key(k)], 2e-4)}

    assert failing(want) == set()
    g = dict(want)
    g["sigma.bias"] = torch.zeros_like(want["sigma.bias"])
    assert failing(g) == {"sigma.bias"}
    g = dict(want)
    g["layers.3.weight"] = want["layers.3.weight"].clone()
    g["layers.3.weight"][32:48] = 0.0
    assert "layers.3.weight[rows 32:48]" in failing(g) and "layers.3.weight[rows 16:32]" not in failing(g)
    g = dict(want)
    w = want["layers.2.weight"]  # successor of skip layer 1: [hidden | encoding] columns
    g["layers.2.weight"] = torch.cat([w[:, D:], w[:, :D]], dim=1)
    assert {"layers.2.weight[enc]", "layers.2.weight[hid]"} <= failing(g)
