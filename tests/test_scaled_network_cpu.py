"""CPU (no GPU): the scaled network of round 4 (FSN_PREC_FP16X3U) on the oracle.
(1) The transformation the packer applies (per-layer powers of two folded into weights / biases / heads,
oracle.scale_state_dict = csrc/mlp_pack.hpp) is EXACT: the scaled network's outputs equal the reference's bit for bit in
float64 and in float32, whatever the exponents.
(2) The arithmetic the kernels then run - three fp16 products with UNSCALED low parts, oracle.split_linear("fp16x3u") - is
float32-grade on the CALIBRATED scaled network for networks whose own activations are 1e-6 ... 1e6 x the default
initialisation's, and is NOT on the unscaled network away from scale 1: the reason the calibration exists."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fsnerf_oracle as O  # noqa: E402

L, D = 8, 256
CFG = dict(n_layers=L, skip=[4], n_freqs=10, n_freqs_dir=4, log_space=True)


def scaled_sd(seed, s):
    """hidden activations s x the default net's, outputs unchanged (tests/test_parity_fp64.py:scaled_sd)."""
    sd = O.init_nerf_state_dict(L, D, [4], 10, 4, seed=seed)
    sd["sigma.weight"] = sd["sigma.weight"] * 64.0
    sd["sigma.bias"] = sd["sigma.bias"] + 3.0
    sd["layers.0.weight"] = sd["layers.0.weight"] * s
    for i in range(L):
        sd[f"layers.{i}.bias"] = sd[f"layers.{i}.bias"] * s
    w = sd["layers.5.weight"].clone()
    w[:, D:] = w[:, D:] * s
    sd["layers.5.weight"] = w
    sd["sigma.weight"] = sd["sigma.weight"] / s
    sd["connection.weight"] = sd["connection.weight"] / s
    return sd


def probe(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=g) * 3.0 - 1.5
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    return x, d


def test_the_scaling_is_an_exact_transformation():
    x, d = probe(300, 1)
    sd = scaled_sd(42, 1.0)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        exps = [int(e) for e in torch.randint(-20, 21, (L + 2,), generator=g)]
        sds = O.scale_state_dict(sd, exps, n_layers=L, skip=[4], d_hidden=D)
        for dt in (torch.float64, torch.float32):
            a = O.nerf_forward({k: v.to(dt) for k, v in sd.items()}, x.to(dt), d.to(dt), **CFG)
            b = O.nerf_forward({k: v.to(dt) for k, v in sds.items()}, x.to(dt), d.to(dt), **CFG)
            assert torch.equal(a, b), (exps, dt)
        # the hidden activations ARE scaled: GEMM g's maximum is 2^e_g x the plain network's
        m0 = O.layer_maxima(sd, x, d, **CFG)
        m1 = O.layer_maxima(sds, x, d, **CFG)
        assert all(abs(b_ / a_ / 2.0 ** e - 1.0) < 1e-12 for a_, b_, e in zip(m0, m1, exps))


@pytest.mark.parametrize("s", [1e-6, 1e-3, 1.0, 1e3, 1e6])
def test_plain_split_is_float32_grade_on_the_calibrated_network(s):
    """The yardstick is the float32 oracle's own error, and the worst of its 1,500 samples depends on the order in which
    the host's BLAS sums a GEMM: MKL takes other kernels on other CPUs (the float32 oracle's worst sample at s = 1e-6 is
    6.3e-6 on one host and 2.5e-6 on another).  The checks therefore run in a child process on MKL's reproducible code
    path (MKL_CBWR=COMPATIBLE, the same on every x86 CPU) with one thread: the same sums on every machine."""
    env = dict(os.environ, MKL_CBWR="COMPATIBLE", MKL_NUM_THREADS="1", OMP_NUM_THREADS="1")
    code = f"import test_scaled_network_cpu as T; T.check_float32_grade({s!r})"
    out = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], capture_output=True,
                         text=True, env=env, cwd=os.path.dirname(os.path.abspath(__file__)), timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]


def check_float32_grade(s):
    x, d = probe(1500, 2)
    xp, dp = probe(400, 9)  # calibration sees OTHER samples than the evaluation
    sd = scaled_sd(42, s)
    exps = O.calibrate_exps(O.layer_maxima(sd, xp, dp, **CFG))
    sds = O.scale_state_dict(sd, exps, n_layers=L, skip=[4], d_hidden=D)
    mx = O.layer_maxima(sds, xp, dp, **CFG)
    assert all(2.0 ** 9 < v <= 2.0 ** 10 for v in mx), mx
    want = O.nerf_forward({k: v.double() for k, v in sd.items()}, x.double(), d.double(), **CFG)
    o32 = O.nerf_forward(sd, x, d, **CFG).double()
    emu = O.nerf_forward(sds, x, d, emulate="fp16x3u", **CFG).double()
    assert bool(torch.isfinite(emu).all())
    den = want[:, 3].abs().clamp_min(1e-2 * float(want[:, 3].abs().max()))
    es, e32 = (emu[:, 3] - want[:, 3]).abs() / den, (o32[:, 3] - want[:, 3]).abs() / den
    # (measured, tools: mean 1.5 x and 99th percentile 1.4 x the float32 oracle's error at every scale - the weights' unscaled
    # low parts are fp16 subnormals for |w| < 0.125, i.e. carry 2^-25 absolute instead of 2^-11 relative; round 3's scaled
    # low parts: 1.0 x.  The single worst of 1,500 samples is noise-dominated: bounded at 6 x.)
    assert float(es.mean()) <= 2.0 * float(e32.mean()) and float(es.quantile(0.99)) <= 2.0 * float(e32.quantile(0.99)) and \
        float(es.max()) <= 6.0 * float(e32.max()), \
        f"s={s:g}: sigma rel. error max {float(es.max()):.2e} p99 {float(es.quantile(0.99)):.2e} mean {float(es.mean()):.2e}, " \
        f"float32 oracle {float(e32.max()):.2e} / {float(e32.quantile(0.99)):.2e} / {float(e32.mean()):.2e}"
    er, er32 = (emu[:, :3] - want[:, :3]).abs(), (o32[:, :3] - want[:, :3]).abs()
    assert float(er.max()) <= 4.0 * float(er32.max()) + 1e-7
    if s <= 1e-3 or s >= 1e6:
        # the same arithmetic on the UNSCALED network: fp16 overflow above (hidden maxima ~3 s), subnormal low parts below
        raw = O.nerf_forward(sd, x, d, emulate="fp16x3u", **CFG).double()
        er_raw = ((raw[:, 3] - want[:, 3]).abs() / den)
        bad = (not bool(torch.isfinite(raw).all())) or float(er_raw.max()) > 10.0 * float(e32.max())
        assert bad, f"s={s:g}: expected the unscaled network to leave float32 grade ({float(er_raw.max()):.2e})"
