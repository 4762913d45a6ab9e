"""The single-pass training modes (train_precision "fp16" / "bf16") entry by entry.  Their own code in every training
kernel - store_pair_parts<false> and the halved row stride in k_train_fwd / k_train_bwd, k_wgrad's !X3 lane offsets,
RSTEP, granule order and half_last, k_heads_wgrad's load_pair, k_input_grad's single-pass instantiations - was covered by
two whole-gradient cosine tests (tests/test_train_step.py::test_single_pass_training_modes_run,
tests/test_input_grad.py::test_single_pass_modes_input_gradients), which a dropped bias gradient, a wrong 16-row block, a
mishandled half tile or a lost tail tile pass.

The calls are the ops-level pair (ops.nerf_train_fwd / nerf_train_bwd / nerf_train_bwd_inputs) without stage arrays
(factors 1) and with a fresh status word, asserted 0 after every call: stateless, deterministic.  References and
yardsticks: tests/test_train_emul_cpu.py (float64 autograd; tests/train_emul_ref.py's restatement of the modes' operand
rounding and its own error).  Networks (8, 256, (4,), 10, 4), (6, 128, (1, 3), 7, 3), (2, 128, (), 10, 4); 300 samples =
two 128-sample tiles and a ragged one.

a. Pinned networks (no ReLU unit can change branch: every pre-activation is 0.5 .. 1.5 from zero), every parameter
   gradient and d_x / d_dirs (one network: the ray form through ray_grad_reduce) against float64 autograd, largest
   absolute error over the tensor's largest entry; weight gradients also per block of 16 output rows and per column
   block (hidden / encoding columns come from different wgrad launches).  Bar: max(4 x the restatement's own error for
   that tensor, 2e-4): the kernel differs from the restatement by float32 accumulation, which moves a few operands by one
   unit of the format (the factor of tests/test_shape_corners_gpu.py); 2e-4 is TRAIN_MODES' fp32-grade bar, for what the
   restatement gets exactly (head biases).  fp16 on 6x128 also with cotangents x 1e-7 and x 1e3 (gradient scaling).
b. Natural networks (test_nerf_gradients_vs_autograd's initialisation, 777 samples, masks differ per sample and units
   near zero change branch): relative L2 error per tensor and column block <= max(4 x the restatement's, 2e-4), finite,
   non-zero wherever float64's is (tensor, column block, 16-row block).  A statistical bar: flips hit other samples in
   the kernel than in the restatement.
c. Placement: one sample with a cotangent at row p of a batch whose other cotangent rows are zero gives, bit for bit,
   the parameter gradients and the d_x / d_dirs row of the one-sample call, and exact zeros in the other rows; 130
   samples with cotangents followed by 170 rows without give the 130-sample call.

Measured on the MI355X.  (a), largest kernel error / restatement error over the tensors and column blocks of a case (bar:
4), and the head biases' own error (bar: 2e-4; the restatement's is 0 .. 6.4e-5):

  net     form, cotangent   fp16                          bf16
  8x256   point             1.20 (layers.2.weight) 7.7e-6   1.04 (layers.4.weight) 1.1e-4
  6x128   point             1.07 (branch.weight)   5.4e-6   1.04 (layers.5.weight) 2.9e-5
  2x128   point             1.08 (layers.1.weight) 2.6e-6   1.07 (layers.1.weight) 3.3e-5
  6x128   rays              1.05 (layers.2.bias)   7.3e-6   1.00 (d_rays_o)        6.4e-5
  6x128   point, x 1e-7     1.07 (branch.weight)   5.3e-6
  6x128   point, x 1e3      1.07 (layers.1.bias)   5.2e-6

The restatement's own errors on these cases are 1.5e-4 .. 4.3e-3 in fp16 (the largest: layers.0.bias of 8x256, whose
dPre_0 reaches fp16's subnormals without per-stage factors - the restatement rounds at the scaled magnitude too) and
9e-4 .. 1.2e-2 in bf16 (tensors and column blocks other than the head biases), so the bars are 6e-4 .. 1.7e-2 and
3.7e-3 .. 4.7e-2.  (b), largest kernel L2 error / restatement L2 error (bar: 4; the restatement's own relative L2 errors
are 3e-4 .. 4.4e-2 in fp16 and 2e-3 .. 1.1e-1 in bf16):

  8x256   fp16 1.04   bf16 1.03        6x128   fp16 1.02   bf16 1.01        2x128   fp16 1.04   bf16 1.04

(c) holds bit for bit in all four cases: every parameter gradient, the sample's d_x / d_dirs row, exact zeros elsewhere.
"""
import pytest
import torch

import test_train_emul_cpu as Y
import train_emul_ref as R
from oracle import fsnerf_oracle as O

pytestmark = pytest.mark.gpu

FLOOR = 2e-4   # tests/test_train_step.py TRAIN_MODES: the fp32-grade bar
FACTOR = 4.0   # tests/test_shape_corners_gpu.py: single-pass kernel against the emulation's own error


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import fs_nerf_amd  # noqa: F401
    from fs_nerf_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def names_of(net):
    from fs_nerf_amd import ops
    return [f"layers.{i}" for i in range(Y.NETS[net][0])] + list(ops.SD_ORDER_TAIL)


def run(dev, net, mode, sd, inputs, c, params_twice=False):
    """One training step of the kernels on `inputs` with cotangent c -> (out, {name: gradient}) on the CPU; the input
    gradients as R.gradients names them.  `params_twice`: nerf_train_bwd as well, whose parameter gradients are those
    of nerf_train_bwd_inputs bit for bit."""
    from fs_nerf_amd import _lib as Lb, ops
    L, D, skip, nf, nfd = Y.NETS[net]
    prec = {"fp16": Lb.FSN_PREC_FP16, "bf16": Lb.FSN_PREC_BF16}[mode]
    desc = ops.make_desc(L, D, skip, O.pe_freqs(nf, True).tolist(), O.pe_freqs(nfd, True).tolist())
    ws, bs = ops.sd_tensor_lists({k: v.to(dev) for k, v in sd.items()}, L)
    c = c.float().to(dev).contiguous()
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    if mode == "fp16":
        assert float(ops.grad_scale_for(c)[0]) == R.grad_scale(c.cpu()), "the restatement's gradient scale is the kernel's"
    if "ri" in inputs:
        rays = tuple(inputs[k].to(dev) for k in ("o", "d", "ri", "t0", "t1"))
        out, work = ops.nerf_train_fwd_rays(desc, prec, ws, bs, *rays, None, None, status=word)
        src = dict(rays=rays)
    else:
        x, d = inputs["x"].to(dev), inputs["d"].to(dev)
        out, work = ops.nerf_train_fwd(desc, prec, ws, bs, x, d, None, None, status=word)
        src = dict(x=x, dirs=d)
    assert int(word.item()) == 0, "forward status"
    plain = None
    if params_twice:
        dW, db = ops.nerf_train_bwd(desc, prec, ws, work, out, c, status=word)
        assert int(word.item()) == 0, "backward status"
        plain = [g.clone() for g in dW] + [g.clone() for g in db]
    dW, db, g_x, g_d = ops.nerf_train_bwd_inputs(desc, prec, ws, work, out, c, status=word, **src)
    assert int(word.item()) == 0, "backward status"
    if plain is not None:
        assert all(torch.equal(a, b) for a, b in zip(plain, list(dW) + list(db))), "nerf_train_bwd != nerf_train_bwd_inputs"
    got = {}
    for n, gw, gb, w in zip(names_of(net), dW, db, ws):
        got[n + ".weight"], got[n + ".bias"] = gw.reshape(w.shape).cpu(), gb.reshape(-1).cpu()
    if "ri" in inputs:
        g_o, g_rd = ops.ray_grad_reduce(g_x, g_d, rays[2], rays[3], rays[4], rays[0].shape[0])
        got["d_rays_o"], got["d_rays_d"] = g_o.cpu(), g_rd.cpu()
    else:
        got["d_x"], got["d_dirs"] = g_x.cpu(), g_d.cpu()
    return out.cpu(), got


# ------------------------------------------------------------------------------------------------ a. pinned, entry by entry
@pytest.mark.parametrize("net,mode,form,cscale", Y.PINNED_CASES)
def test_pinned_network_gradients_entry_by_entry(dev, net, mode, form, cscale):
    case = Y.pinned(net, mode, form, cscale)
    want, yard = case["want"], case["yard"]
    out, got = run(dev, net, mode, case["sd"], case["inputs"], case["c"], params_twice=True)
    assert set(got) == set(want)
    assert all(bool(torch.isfinite(g).all()) for g in got.values())
    m = R.entry_metrics(got, want, Y.NETS[net])
    assert set(m) == set(yard)
    fails, worst, worst_key, head_bias = [], 0.0, None, 0.0
    for k in sorted(m):
        base = R.base_key(k)
        bar = max(FACTOR * yard[base], FLOOR)
        if k == base:
            print(f"{net} {mode} {form} x{cscale:g} {k}: kernel {m[k]:.2e}, restatement {yard[k]:.2e}, bar {bar:.2e}")
            if k in ("sigma.bias", "rgb.bias"):
                head_bias = max(head_bias, m[k])
            elif m[k] / yard[k] > worst:
                worst, worst_key = m[k] / yard[k], k
        if not m[k] <= bar:
            fails.append(f"{k}: {m[k]:.3e} > {bar:.3e} (restatement {yard[base]:.3e})")
    print(f"FIGURE a {net} {mode} {form} x{cscale:g}: kernel / restatement at most {worst:.2f} ({worst_key}); head biases {head_bias:.1e}")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ b. natural, tensor by tensor
@pytest.mark.parametrize("mode", Y.MODES)
@pytest.mark.parametrize("net", list(Y.NETS))
def test_natural_network_gradients_tensor_by_tensor(dev, net, mode):
    case = Y.natural(net, mode)
    want, yard = case["want"], case["yard"]
    out, got = run(dev, net, mode, case["sd"], case["inputs"], case["c"])
    assert set(got) == set(want)
    m = R.l2_metrics(got, want, Y.NETS[net])
    assert set(m) == set(yard)
    fails, worst, worst_key = [], 0.0, None
    for k in sorted(m):
        err, n_got, n_want, finite = m[k]
        if not finite:
            fails.append(f"{k}: not finite")
        if n_want > 0 and not n_got > 0:
            fails.append(f"{k}: zero where float64's gradient is not")
        if "[rows" in k:
            continue
        bar = max(FACTOR * yard[k][0], FLOOR)
        print(f"{net} {mode} {k}: kernel L2 {err:.2e}, restatement {yard[k][0]:.2e}, bar {bar:.2e}")
        if yard[k][0] > 0 and err / yard[k][0] > worst:
            worst, worst_key = err / yard[k][0], k
        if not err <= bar:
            fails.append(f"{k}: L2 {err:.3e} > {bar:.3e} (restatement {yard[k][0]:.3e})")
    print(f"FIGURE b {net} {mode}: kernel / restatement at most {worst:.2f} ({worst_key})")
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ c. placement
PLACES = [(0, 1), (0, 300), (15, 300), (16, 300), (127, 300), (128, 300), (128, 129), (299, 300)]


def _differing(a, b, keys):
    return [k for k in keys if not torch.equal(a[k], b[k])]


@pytest.mark.parametrize("mode", Y.MODES)
@pytest.mark.parametrize("net", ["8x256", "6x128"])
def test_a_samples_contribution_does_not_depend_on_its_place(dev, net, mode):
    """Expected bit for bit: a zero cotangent row gives exact-zero dPre, products of two 16-bit operands are exact in
    float32, the split-K reduce adds zeros, grad_scale_for sees the same maximum."""
    case = Y.pinned(net, mode)
    x, d, c = case["inputs"]["x"], case["inputs"]["d"], case["c"]
    params = sorted(case["sd"])
    ref = None
    for p, n in PLACES:
        xb, db, cb = x[:n].clone(), d[:n].clone(), torch.zeros(n, 4)
        xb[p], db[p], cb[p] = x[0], d[0], c[0]
        out, got = run(dev, net, mode, case["sd"], {"x": xb, "d": db}, cb)
        if ref is None:
            assert (p, n) == (0, 1)
            ref = got
            assert all(float(got[k].abs().max()) > 0 for k in params + ["d_x", "d_dirs"])
            continue
        diff = _differing(got, ref, params)
        assert not diff, f"row {p} of {n}: {diff} differ from the one-sample call"
        for k in ("d_x", "d_dirs"):
            assert torch.equal(got[k][p], ref[k][0]), f"row {p} of {n}: {k} of the sample"
            rest = torch.cat([got[k][:p], got[k][p + 1:]])
            assert int((rest != 0).sum()) == 0, f"row {p} of {n}: {k} of rows without a cotangent"
    # 130 samples with cotangents, then 170 rows without
    n0 = 130
    _, short = run(dev, net, mode, case["sd"], {"x": x[:n0].clone(), "d": d[:n0].clone()}, c[:n0].clone())
    cb = c.clone()
    cb[n0:] = 0.0
    _, full = run(dev, net, mode, case["sd"], {"x": x, "d": d}, cb)
    diff = _differing(full, short, params)
    assert not diff, f"130 of 300: {diff} differ from the 130-sample call"
    for k in ("d_x", "d_dirs"):
        assert torch.equal(full[k][:n0], short[k]) and int((full[k][n0:] != 0).sum()) == 0, k
