"""Which HIP entry point `render_rays` / `render_frame` reach, pinned on the CPU.  A dispatch change that keeps the
outputs bitwise equal but takes another launch route (the unfused sequence instead of one launch, the plain sampler
instead of the fused one) passes every numerical test; this one fails on it.

The calls are intercepted at the `ops` boundary: every launch entry point the routes can reach is replaced by a stub
that records its name and the `camera` / `want_extras` / `status` arguments, then raises; `NeRF.packed` /
`NeRF.packed_cull` record their name and return a dummy.  The expected route of every case is spelled out below
(`expected_rays` / `expected_frame`) over the cross product of the attributes the choice reads."""
import itertools

import pytest
import torch
from torch import nn

from fs_nerf_amd import ops
from fs_nerf_amd.core.models import NeRF
from fs_nerf_amd.render import rendering as Rm
from fs_nerf_amd.render.occgrid import OccGridEstimator
from fs_nerf_amd.utils import utilities as U

ENTRIES = ("render_fused", "render_occ_fused", "sample_fused", "occ_sample_fused", "stratified_edges", "occgrid_march")
OCC_PRECISIONS = ("fp16x3", "bf16x3", "fp16", "bf16")            # the one-launch occupancy kernel
SAMPLER_PRECISIONS = ("fp16x3", "bf16x3", "fp16", "bf16", "fp16x2")  # the fused stratified sampler
STEP_FITS, STEP_TOO_FINE = 5e-3, 1e-3  # max_steps 1042 / 5198 of the box below, against FUSED_OCC_MAX_STEPS 2048
AABB = [-1.5, -1.5, -1.5, 1.5, 1.5, 1.5]


class Reached(Exception):
    pass


@pytest.fixture
def log(monkeypatch):
    calls = []

    def entry(name):
        def stub(*args, **kw):
            calls.append((name, kw.get("camera") is not None, kw.get("want_extras"), kw.get("status") is not None))
            raise Reached(name)
        return stub

    def packer(name):
        def stub(self, *args, **kw):
            calls.append((name,))
            return object()
        return stub

    def get_rays(pose, hwf, device):
        calls.append(("get_rays",))
        H, W, _ = hwf
        return torch.zeros(H, W, 3, device=device), torch.ones(H, W, 3, device=device)

    def to_ndc(rays_o, rays_d, hwf, near):
        calls.append(("to_ndc",))
        return rays_o, rays_d

    for name in ENTRIES:
        monkeypatch.setattr(ops, name, entry(name))
    monkeypatch.setattr(NeRF, "packed", packer("packed"))
    monkeypatch.setattr(NeRF, "packed_cull", packer("packed_cull"))
    monkeypatch.setattr(U, "get_rays", get_rays)
    monkeypatch.setattr(U, "to_ndc", to_ndc)
    return calls


def nerf(precision="fp16x3", cull=None):
    m = NeRF(3, 3, 2, 16, (), precision=precision, pos_fn={"n_freqs": 2, "log_space": True},
             dir_fn={"n_freqs": 1, "log_space": True})
    m.cull_precision = cull
    return m


def estimators():
    return {"stratified": Rm.StratifiedEstimator(2.0, 6.0, 8, 16),
            "stratified-coarse": Rm.StratifiedEstimator(2.0, 6.0, 8, 0),
            "occgrid": OccGridEstimator(AABB, resolution=16)}


def is_nerf(m):
    return isinstance(m, NeRF)


def occ_one_launch_ok(est, model, model_fine, step):
    return isinstance(est, OccGridEstimator) and is_nerf(model) and model_fine is None and \
        model.precision in OCC_PRECISIONS and est.max_steps(step) <= Rm.FUSED_OCC_MAX_STEPS


def expected_rays(est, model, model_fine, grad, extras, n_rays, step):
    """The route of render_rays as a list of the recorded calls up to the first launch."""
    fine = model_fine if model_fine is not None else model
    cull = is_nerf(model) and model.cull_precision is not None
    f16 = is_nerf(model) and model.precision in ("fp16x3", "fp16", "fp16x2")
    if not grad and not cull and occ_one_launch_ok(est, model, model_fine, step):
        if not extras:
            return [("packed",), ("render_occ_fused", False, False, False)]
        if Rm.FUSED_OCC_EXTRAS and n_rays * est.max_steps(step) <= Rm.FUSED_OCC_EXTRAS_MAX_SLOTS:
            return [("packed",), ("render_occ_fused", False, True, False)]
    strat = isinstance(est, Rm.StratifiedEstimator)
    if strat and is_nerf(model) and is_nerf(fine) and not grad:
        return [("packed",)] * (2 if est.n_importance > 0 else 1) + [("render_fused", False, extras, False)]
    if strat and est.n_importance > 0 and is_nerf(model) and model.precision in SAMPLER_PRECISIONS:
        return [("packed",), ("sample_fused", False, None, grad and f16)]
    if Rm.FUSED_OCC_SAMPLER and (n_rays >= max(1, Rm.FUSED_OCC_SAMPLER_MIN_RAYS) or cull) and \
            occ_one_launch_ok(est, model, None, step):  # (model_fine does not block the sampler)
        if cull:
            return [("packed_cull",), ("occ_sample_fused", False, None, False)]
        return [("packed",), ("occ_sample_fused", False, None, grad and f16)]
    return [("stratified_edges" if strat else "occgrid_march", False, None, False)]


def expected_frame(est, model, model_fine, grad, ndc, n_pixels, step):
    fine = model_fine if model_fine is not None else model
    cull = is_nerf(model) and model.cull_precision is not None
    fused = isinstance(est, Rm.StratifiedEstimator) and is_nerf(model) and is_nerf(fine) and not grad
    if fused and not ndc:
        return [("packed",)] * (2 if est.n_importance > 0 else 1) + [("render_fused", True, False, False)]
    if not grad and not ndc and not cull and occ_one_launch_ok(est, model, model_fine, step):
        return [("packed",), ("render_occ_fused", True, False, False)]
    pre = [("get_rays",)] + ([("to_ndc",)] if ndc else [])
    return pre + expected_rays(est, model, model_fine, grad, False, n_pixels, step)


def run(log, fn):
    del log[:]
    with pytest.raises(Reached):
        fn()
    return list(log)


def modes(model, model_fine, grad):
    """grad: training mode with parameters that require gradients under autograd; else no_grad (eval mode)."""
    for m in (model, model_fine):
        if m is not None:
            m.train(grad)
    return torch.enable_grad() if grad else torch.no_grad()


def nets():
    """(label, model, model_fine) for NeRF / plain models over the precisions and the cull mode the choice reads."""
    plain = lambda: nn.Linear(3, 4)
    models = [(f"nerf-{p}-{c}", lambda p=p, c=c: nerf(p, c)) for p in ("fp16x3", "fp16x2", "bf16x3")
              for c in (None, "bf16")] + [("plain", plain)]
    fines = [("none", lambda: None), ("nerf", nerf), ("plain", plain)]
    for (lm, mk_m), (lf, mk_f) in itertools.product(models, fines):
        yield f"{lm}/fine-{lf}", mk_m(), mk_f()


@pytest.mark.parametrize("sampler_on", [True, False])
def test_render_rays_routes(log, monkeypatch, sampler_on):
    monkeypatch.setattr(Rm, "FUSED_OCC_SAMPLER", sampler_on)
    ests = estimators()
    wrong, n = [], 0
    for label, model, model_fine in nets():
        for (ek, est), grad, extras, n_rays, step in itertools.product(
                ests.items(), (False, True), (False, True), (64, Rm.FUSED_OCC_SAMPLER_MIN_RAYS), (STEP_FITS, STEP_TOO_FINE)):
            rays_o, rays_d = torch.zeros(n_rays, 3), torch.ones(n_rays, 3)
            want = expected_rays(est, model, model_fine, grad, extras, n_rays, step)
            with modes(model, model_fine, grad):
                got = run(log, lambda: Rm.render_rays(rays_o, rays_d, est, model, train=grad, render_step_size=step,
                                                      device="cpu", model_fine=model_fine, want_extras=extras))
            n += 1
            if got != want:
                wrong.append((label, ek, grad, extras, n_rays, step, got, want))
    assert n > 1000
    assert not wrong, f"{len(wrong)} of {n} cases took another route, e.g. {wrong[:3]}"


def test_render_rays_occ_extras_limits(log, monkeypatch):
    """FUSED_OCC_EXTRAS / FUSED_OCC_EXTRAS_MAX_SLOTS / FUSED_OCC_SAMPLER_MIN_RAYS are read at call time."""
    est, model = OccGridEstimator(AABB, resolution=16), nerf()
    model.eval()
    rays_o, rays_d = torch.zeros(64, 3), torch.ones(64, 3)
    call = lambda: Rm.render_rays(rays_o, rays_d, est, model, render_step_size=STEP_FITS, device="cpu")
    with torch.no_grad():
        assert run(log, call)[-1] == ("render_occ_fused", False, True, False)
        monkeypatch.setattr(Rm, "FUSED_OCC_EXTRAS_MAX_SLOTS", 64 * est.max_steps(STEP_FITS) - 1)
        assert run(log, call)[-1] == ("occgrid_march", False, None, False)
        monkeypatch.setattr(Rm, "FUSED_OCC_SAMPLER_MIN_RAYS", 64)
        assert run(log, call)[-1] == ("occ_sample_fused", False, None, False)
        monkeypatch.setattr(Rm, "FUSED_OCC_EXTRAS_MAX_SLOTS", 1 << 26)
        monkeypatch.setattr(Rm, "FUSED_OCC_EXTRAS", False)
        assert run(log, call)[-1] == ("occ_sample_fused", False, None, False)


@pytest.mark.parametrize("sampler_on", [True, False])
def test_render_frame_routes(log, monkeypatch, sampler_on):
    monkeypatch.setattr(Rm, "FUSED_OCC_SAMPLER", sampler_on)
    # a device WITH an index: the one-launch paths would ask torch.cuda for the current device otherwise
    dev = torch.device("cpu", 0)
    ests = estimators()
    H, W = 8, 8
    wrong, n = [], 0
    for label, model, model_fine in nets():
        for (ek, est), grad, ndc, step in itertools.product(ests.items(), (False, True), (False, True),
                                                             (STEP_FITS, STEP_TOO_FINE)):
            want = expected_frame(est, model, model_fine, grad, ndc, H * W, step)
            with modes(model, model_fine, grad):
                got = run(log, lambda: Rm.render_frame((H, W, 10.0), 2.0, 6.0, torch.eye(4), 4096, est, model, train=grad,
                                                       ndc=ndc, render_step_size=step, device=dev, model_fine=model_fine))
            n += 1
            if got != want:
                wrong.append((label, ek, grad, ndc, step, got, want))
    assert n > 300
    assert not wrong, f"{len(wrong)} of {n} cases took another route, e.g. {wrong[:3]}"
