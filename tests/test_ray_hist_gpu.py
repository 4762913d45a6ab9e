"""GPU: the neighbouring-ray KL (csrc/ray_hist.hip: fsn_ray_hist_*, fsn_patch_nkl_*) through ops.py and core/loss.py,
against the three references of tests/ray_hist_ref.py.

Inputs: the float32 outputs of ops.composite_packed on tests/composite_ref.ragged_case(S), S in {5, 64, 65, 192} (fewer
samples than lanes, one per lane, a ragged last lane, three per lane; 70 rays, ray 3 empty, ray 7 with every value
exactly 0, about 5 % negative entries); bins in {1, 7, 64, 65, 200} (fewer bins than lanes, one per lane, ragged,
several per lane; with S = 5 a sample spans many bins); the ranges [2, 7] (covers every sample) and [3, 5] (samples
straddle both ends).

Bit for bit: the unnormalised histogram against the float32 NumPy loop; a row subset against the full call; two calls
against each other.  Against float64: the reference takes the same float32 tensors (and the GPU's own float32 P for the
patch term, so that only that term's arithmetic is compared) and the float32 edges as given.  Metric:
test_train_step._rel, max |a - b| / max |b|; bars 1e-5 (values) and 2e-4 (gradients), the project's bars on this
skeleton (float32 on the CPU: 6.9e-7 / 1.6e-7 for the histogram, 2.4e-7 / 1.2e-6 for the patch term).  Ray 7 (s = 0: its
gradient is of order 1 / eps) is measured against its own maximum, apart from the rest.

One case has no gradient to measure against: one bin over the covering range.  There every sample has f = 1 and
P = s / (s + eps), so d u = G (1 - P) / (s + eps): the two terms cancel to about 1e-10 of their size, which is below
float32's resolution of either (P rounds to 1).  A float32 difference is accurate relative to its operands, not to its
result, so in that one case the gradient error is measured against the largest term, max |G_r| / (s_r + eps), with
the same 2e-4 bar.  The patch term's histograms are taken over [3, 5] for the same reason (over [2, 7] one bin gives
P = 1 on every ray and every D is rounding noise).

Measured on the MI355X (the tests print the figures): see DESIGN.md 6.1, "Neighbouring-ray KL"."""
import functools

import pytest
import torch

import fs_nerf_amd  # noqa: F401
from oracle import fsnerf_oracle as O

import composite_ref as CR
import ray_hist_ref as RH
from test_train_step import _rel

SIZES = [5, 64, 65, 192]
BINS = [1, 7, 64, 65, 200]
RANGES = [(2.0, 7.0), (3.0, 5.0)]
BK = torch.tensor([1.0, 0.5, 0.25])
TOL_GRAD, TOL_FWD = 2e-4, 1e-5
THRESHOLD = 0.1
MASKED_RAYS = (CR.EMPTY_RAY, CR.ZERO_RAY, 12)
PATCH_CASES = [((2, 5, 7), b) for b in BINS] + [((1, 2, 2), 65), ((3, 4, 4), 65), ((2, 1, 7), 65), ((2, 7, 1), 65)]


@functools.lru_cache(maxsize=None)
def _setup(S):
    """the case, its tensors on the device, the GPU forward (float32) and its CPU copy: built once per size, never
    modified"""
    from fs_nerf_amd import ops
    dev = torch.device("cuda:0")
    case = CR.ragged_case(S)
    g = {k: case[k].to(dev) for k in ("sig", "rgb", "t0", "t1", "ri")}
    _, opacity, _, ex = ops.composite_packed(g["sig"], g["rgb"], g["t0"], g["t1"], g["ri"], case["R"], BK)
    fwd = dict(opacity=opacity, weights=ex["weights"], alphas=ex["alphas"])
    cpu = {k: v.detach().cpu() for k, v in fwd.items()}
    assert case["R"] == 70 and int((case["ri"] == CR.EMPTY_RAY).sum()) == 0
    assert bool((cpu["weights"][case["ri"] == CR.ZERO_RAY] == 0).all()) and int((cpu["weights"] < 0).sum()) > 0
    return case, g, fwd, cpu


@functools.lru_cache(maxsize=None)
def _cotangent(S, bins):
    return torch.randn(70, bins, generator=torch.Generator().manual_seed(1000 + 7 * S + bins))


def _bits_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _hist(S, bins, rng, G=None, normalize=True, rays=None):
    """one call of ops.ray_histogram on the case's weights (and its backward under the cotangent G) -> (leaf, out)"""
    from fs_nerf_amd import ops
    case, g, fwd, _ = _setup(S)
    v = fwd["weights"].detach().clone().requires_grad_(True)
    out = ops.ray_histogram(v, g["t0"], g["t1"], g["ri"], case["R"], bins=bins, t_min=rng[0], t_max=rng[1],
                            normalize=normalize, rays=rays)
    if G is not None:
        (out * G.to(out.device)).sum().backward()
    return v, out


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("rng", RANGES)
def test_histogram_bits_value_gradient_and_determinism(S, bins, rng):
    """H equals the float32 NumPy loop bit for bit; P within 1e-5 and both gradients within 2e-4 of float64; ray 7 against
    its own maximum, its row of P exactly 0; rows sum to at most 1; gradient bitwise 0 at negative entries, passing where
    v == 0; two calls are equal bit for bit.
    Measured on the MI355X, all 40 combinations: P <= 6.0e-7, d_values <= 2.1e-7 (one bin over [2, 7], against the
    largest term: <= 4.1e-7; max |reference| there 1.9e-9), the unnormalised gradient <= 1.8e-7, ray 7 <= 3.0e-7 of its
    own maximum (5.1e8 ... 2.7e10; the other rays' entries are at most 5.0)."""
    case, g, fwd, cpu = _setup(S)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    G = _cotangent(S, bins)
    edges = RH.edges_f32(bins, *rng)
    w32 = cpu["weights"]
    w64, t0, t1 = w32.double(), case["t0"].double(), case["t1"].double()
    seven, neg = ri == CR.ZERO_RAY, w32 < 0

    # unnormalised: bit for bit, and its gradient (no cancellation in it at any size)
    vH, H = _hist(S, bins, rng, G, normalize=False)
    assert H.shape == (R, bins) and H.requires_grad
    loop = torch.from_numpy(RH.hist_f32_loop(w32.numpy(), case["t0"].numpy(), case["t1"].numpy(), ri.numpy(), R, bins, *rng))
    assert torch.equal(H.detach().cpu().view(torch.int32), loop.view(torch.int32))
    ref_gH = RH.hist_grad(w64, t0, t1, ri, R, edges, G.double(), normalize=False)
    e_gH = _rel(vH.grad, ref_gH)
    assert e_gH < TOL_GRAD, e_gH

    # normalised
    v, P = _hist(S, bins, rng, G)
    ref = RH.hist_value(w64, t0, t1, ri, R, edges)
    ref_g = RH.hist_grad(w64, t0, t1, ri, R, edges, G.double())
    ev = _rel(P, ref)
    grad = v.grad.cpu()
    if bins == 1 and rng == RANGES[0]:  # (the module docstring: the two terms cancel; measured against the terms)
        terms = (G[:, 0].double().abs() / (CR.seg_sum(torch.clamp(w64, min=0.0), ri, R) + 1e-10))[ri]
        eg = float((grad.double() - ref_g)[~seven].abs().max() / terms[~seven].max())
    else:
        eg = _rel(grad[~seven], ref_g[~seven])
    e7 = _rel(grad[seven], ref_g[seven])
    print(f"S={S} bins={bins} range={rng}: P={ev:.3e} d_values={eg:.3e} ray7={e7:.3e} unnormalised d_values={e_gH:.3e} "
          f"(max |reference|: ray 7 {float(ref_g[seven].abs().max()):.3e}, the rest {float(ref_g[~seven].abs().max()):.3e})")
    assert bool(torch.isfinite(P).all()) and bool(torch.isfinite(v.grad).all())
    assert ev < TOL_FWD and eg < TOL_GRAD and e7 < TOL_GRAD, (ev, eg, e7)
    assert float(ref_g[seven].abs().max()) > 1e8  # (why ray 7 is measured apart)
    assert _bits_zero(P.detach()[CR.EMPTY_RAY]) and _bits_zero(P.detach()[CR.ZERO_RAY])
    assert float(P.detach().sum(dim=1).max()) <= 1.0 + 1e-5 and float(P.detach().min()) >= 0.0
    assert int(neg.sum()) > 0 and _bits_zero(v.grad[neg.to(dev)]) and _bits_zero(vH.grad[neg.to(dev)])
    inside = seven & (case["t1"] > float(edges[0])) & (case["t0"] < float(edges[-1]))  # v == 0 and f > 0 somewhere
    assert int(inside.sum()) > 0 and bool((grad[inside] != 0).all()) and bool((vH.grad.cpu()[inside] != 0).all())

    v2, P2 = _hist(S, bins, rng, G)
    assert torch.equal(P2, P) and torch.equal(v2.grad, v.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 65])
@pytest.mark.parametrize("bins", [7, 200])
def test_histogram_row_subset(S, bins):
    """rays=(first, count): the matching rows of the full call bit for bit - an empty ray first, the all-zero ray inside,
    a count that is no multiple of the four rays of a block, the last ray - and every other sample's gradient bitwise 0"""
    case, g, fwd, cpu = _setup(S)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    rng = RANGES[1]
    G = _cotangent(S, bins)
    v_full, P_full = _hist(S, bins, rng)
    for first, count in ((3, 10), (0, 1), (41, 29), (17, 0)):
        Gs = torch.zeros_like(G)
        Gs[first:first + count] = G[first:first + count]
        v_ref, P_ref = _hist(S, bins, rng, Gs)
        v, P = _hist(S, bins, rng, G[first:first + count], rays=(first, count))
        assert P.shape == (count, bins) and torch.equal(P, P_full[first:first + count]) and torch.equal(P_ref, P_full)
        other = ((ri < first) | (ri >= first + count)).to(dev)
        assert int(other.sum()) > 0 and _bits_zero(v.grad[other])
        assert torch.equal(v.grad[~other], v_ref.grad[~other])
        if count:
            assert float(v.grad.abs().max()) > 0


@pytest.mark.gpu
def test_histogram_of_alphas_unsorted_samples_and_bad_bounds():
    """the alphas, as InfoNeRF takes them; a ray's samples in reversed order (the kernel does not need them sorted); a
    zero-width, a reversed, a NaN and an infinite sample: no mass, gradient bitwise 0 - all bit for bit against the
    float32 loop"""
    from fs_nerf_amd import ops
    case, g, fwd, cpu = _setup(65)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    t0, t1, a = case["t0"].clone(), case["t1"].clone(), cpu["alphas"].clone()
    for r in (5, 20):  # reverse the samples of two rays
        sel = torch.nonzero(ri == r).reshape(-1)
        t0[sel], t1[sel], a[sel] = t0[sel.flip(0)], t1[sel.flip(0)], a[sel.flip(0)]
    bad = torch.nonzero(ri == 30).reshape(-1)[:4]
    t1[bad[0]] = t0[bad[0]]
    t0[bad[1]], t1[bad[1]] = t1[bad[1]].clone(), t0[bad[1]].clone()
    t0[bad[2]] = float("nan")
    t1[bad[3]] = float("inf")
    a[bad] = 0.5
    v = a.to(dev).requires_grad_(True)
    H = ops.ray_histogram(v, t0.to(dev), t1.to(dev), g["ri"], R, bins=65, t_min=3.0, t_max=5.0, normalize=False)
    loop = torch.from_numpy(RH.hist_f32_loop(a.numpy(), t0.numpy(), t1.numpy(), ri.numpy(), R, 65, 3.0, 5.0))
    assert torch.equal(H.detach().cpu().view(torch.int32), loop.view(torch.int32)) and float(loop.max()) > 0
    P = ops.ray_histogram(v, t0.to(dev), t1.to(dev), g["ri"], R, bins=65, t_min=3.0, t_max=5.0)
    G = _cotangent(65, 65)
    (P * G.to(dev)).sum().backward()
    ref_g = RH.hist_grad(a.double(), t0.double(), t1.double(), ri, R, RH.edges_f32(65, 3.0, 5.0), G.double())
    seven = ri == CR.ZERO_RAY
    assert _bits_zero(v.grad[bad.to(dev)]) and bool(torch.isfinite(v.grad).all())
    assert _rel(v.grad.cpu()[~seven], ref_g[~seven]) < TOL_GRAD
    assert _rel(P, RH.hist_value(a.double(), t0.double(), t1.double(), ri, R, RH.edges_f32(65, 3.0, 5.0))) < TOL_FWD


def _patch_mask(n):
    c = torch.ones(n, dtype=torch.bool)
    for r in MASKED_RAYS:
        if r < n:
            c[r] = False
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("shape,bins", PATCH_CASES)
@pytest.mark.parametrize("masked", [False, True])
def test_patch_kl_value_gradient_and_determinism(shape, bins, masked):
    """P = the GPU's own float32 histograms of the first B Ph Pw rays over [3, 5], viewed as patches; the float64
    reference takes that P.  Values within 1e-5, gradients within 2e-4; the mask switches off rays 3, 7 and 12: a pair
    with a masked pixel has value and gradient bitwise 0; contiguous and as a strided view; two calls bit for bit.
    Measured on the MI355X: values <= 5.4e-7, gradients <= 1.3e-7."""
    from fs_nerf_amd import ops
    B, Ph, Pw = shape
    n = B * Ph * Pw
    dev = torch.device("cuda:0")
    _, P70 = _hist(65, bins, RANGES[1])
    P_dev = P70.detach()[:n].reshape(B, Ph, Pw, bins)
    P64 = P_dev.cpu().double()
    c = _patch_mask(n).reshape(B, Ph, Pw) if masked else None
    Gp = torch.randn(B, Ph, Pw, generator=torch.Generator().manual_seed(n + bins))
    ref = RH.nkl_value(P64, c)
    ref_g = RH.nkl_grad(P64, Gp.double(), c)

    def run(strided=False):
        if strided:
            big = torch.zeros(B, Ph, Pw, 2 * bins + 1, device=dev)
            big[..., 1::2] = P_dev
            leaf = big.requires_grad_(True)
            P = leaf[..., 1::2]
            assert not P.is_contiguous() or bins == 1
        else:
            leaf = P = P_dev.clone().requires_grad_(True)
        out = ops.patch_neighbor_kl(P, None if c is None else c.to(dev))
        (out * Gp.to(dev)).sum().backward()
        return leaf, out

    leaf, out = run()
    assert out.shape == (B, Ph, Pw) and leaf.grad.shape == (B, Ph, Pw, bins)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(leaf.grad).all())
    ev, eg = _rel(out, ref), _rel(leaf.grad, ref_g)
    print(f"patches {shape} bins={bins} masked={masked}: value={ev:.3e} d_P={eg:.3e} (max |reference| "
          f"{float(ref.abs().max()):.3e} / {float(ref_g.abs().max()):.3e}; pairs {RH.pair_count(c, shape)})")
    assert float(ref.abs().max()) > 0 and ev < TOL_FWD and eg < TOL_GRAD, (ev, eg)
    if masked:
        off = (~c).to(dev)
        assert int(off.sum()) >= 1 and _bits_zero(leaf.grad[off]) and _bits_zero(out.detach()[off])
        right, down = RH._pair_masks(c, shape, torch.float64)
        owns = torch.zeros(B, Ph, Pw, dtype=torch.bool)
        owns[:, :, :-1] |= right
        owns[:, :-1] |= down
        assert _bits_zero(out.detach()[(~owns).to(dev)])  # a pixel that owns no counted pair
        takes_part = owns.clone()
        takes_part[:, :, 1:] |= right
        takes_part[:, 1:] |= down
        assert _bits_zero(leaf.grad[(~takes_part).to(dev)])
    leaf2, out2 = run()
    assert torch.equal(out2, out) and torch.equal(leaf2.grad, leaf.grad)
    big, out3 = run(strided=True)
    assert torch.equal(out3, out) and torch.equal(big.grad[..., 1::2], leaf.grad) and _bits_zero(big.grad[..., 0::2])


@pytest.mark.gpu
def test_empty_inputs_and_a_single_pixel():
    """N == 0: rows of zeros and an empty gradient; no rows, no patches: empty outputs; (1, 1, 1) has no pair: 0"""
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import NeighborRayKLLoss
    dev = torch.device("cuda:0")
    e = torch.zeros(0, device=dev)
    ei = torch.zeros(0, device=dev, dtype=torch.int64)
    v = e.clone().requires_grad_(True)
    out = ops.ray_histogram(v, e, e, ei, 4, bins=7, t_min=2.0, t_max=6.0)
    assert out.shape == (4, 7) and _bits_zero(out.detach())
    out.sum().backward()
    assert v.grad.shape == (0,)
    assert ops.ray_histogram(e, e, e, ei, 0, bins=7, t_min=2.0, t_max=6.0).shape == (0, 7)
    case, g, fwd, _ = _setup(5)
    assert ops.ray_histogram(fwd["weights"], g["t0"], g["t1"], g["ri"], 70, bins=7, t_min=2.0, t_max=6.0, rays=(9, 0)).shape == (0, 7)
    assert ops.patch_neighbor_kl(torch.zeros(0, 4, 4, 8, device=dev)).shape == (0, 4, 4)
    P = torch.rand(1, 1, 1, 8, device=dev).requires_grad_(True)
    one = ops.patch_neighbor_kl(P)
    one.sum().backward()
    assert one.shape == (1, 1, 1) and _bits_zero(one.detach()) and _bits_zero(P.grad)
    w = fwd["weights"].detach().clone().requires_grad_(True)
    loss = NeighborRayKLLoss(8, t_min=2.0, t_max=7.0)(w, g["t0"], g["t1"], g["ri"], 70, (1, 1, 1), first_ray=20)
    loss.backward()
    assert float(loss.detach()) == 0.0 and _bits_zero(w.grad)


def _chain_cpu(case, dtype, edges, shape, c):
    """sigmas -> oracle.rendering_packed -> weights -> the restatement of NeighborRayKLLoss, on the CPU in `dtype`
    -> d loss / d sigmas"""
    sig = case["sig"].detach().to(dtype).clone().requires_grad_(True)  # (never the cached case's own tensor)
    rgb = case["rgb"].to(dtype)
    t0, t1, ri, R = case["t0"].to(dtype), case["t1"].to(dtype), case["ri"], case["R"]
    _, _, _, ex = O.rendering_packed(t0, t1, ri, R, lambda a, b, i: (rgb, sig), BK.to(dtype))
    RH.loss_value(ex["weights"], t0, t1, ri, R, edges, shape, c=c).backward()
    return sig.grad


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 65])
@pytest.mark.parametrize("bins", [7, 64, 65, 200])
def test_loss_through_the_compositor(S, bins):
    """rendering(full_grad=True) on leaf sigmas, NeighborRayKLLoss of the weights over [2, 7] on the 70 rays as (2, 5, 7)
    patches, masked by opacity: d_sigmas against float64 autograd through oracle.rendering_packed and the restatement.
    (One bin is left to the operator's own tests: over a covering range P = 1 on every ray and the true gradient is
    rounding noise.)  No bar can be derived in advance - 1 / (q + eps) meets bins near zero - so, by the project's rule
    for such chains, the GPU error may be at most 4 x the error of the same chain in float32 torch on the CPU.  The
    test prints both figures.
    Measured, MI355X / float32 on the CPU: S = 5: 2.95e-6 / 3.04e-6 (7 bins), 1.52e-6 / 1.70e-6 (64), 1.65e-6 / 1.57e-6
    (65), 1.58e-6 / 1.58e-6 (200); S = 65: 3.16e-7 / 2.16e-7, 6.63e-6 / 6.33e-6, 6.75e-6 / 6.42e-6, 2.04e-5 / 2.05e-5."""
    from fs_nerf_amd.core.loss import NeighborRayKLLoss
    from fs_nerf_amd.render import rendering as Rm
    case, g, fwd, cpu = _setup(S)
    R, dev, shape = case["R"], g["sig"].device, (2, 5, 7)
    op64 = CR.forward64(case, BK)["opacity"].reshape(-1)
    assert float((op64 - THRESHOLD).abs().min()) > 1e-3  # the mask is the same in every precision
    c = (op64 > THRESHOLD).reshape(shape)
    assert not bool(c.reshape(-1)[CR.ZERO_RAY]) and not bool(c.reshape(-1)[CR.EMPTY_RAY]) and int(c.sum()) > 40
    edges = RH.edges_f32(bins, *RANGES[0])
    ref = _chain_cpu(case, torch.float64, edges, shape, c)
    e32 = _rel(_chain_cpu(case, torch.float32, edges, shape, c), ref)
    sg, rg = g["sig"].clone().requires_grad_(True), g["rgb"].clone().requires_grad_(True)
    _, opacity, _, ex = Rm.rendering(g["t0"], g["t1"], g["ri"], R, lambda a, b, i: (rg, sg), BK.to(dev), full_grad=True)
    assert torch.equal(opacity.detach().cpu().reshape(-1) > THRESHOLD, c.reshape(-1))
    loss = NeighborRayKLLoss(bins, t_min=RANGES[0][0], t_max=RANGES[0][1], threshold=THRESHOLD)(
        ex["weights"], g["t0"], g["t1"], g["ri"], R, shape, opacity=opacity)
    loss.backward()
    e_gpu = _rel(sg.grad, ref)
    print(f"S={S} bins={bins} through the compositor: d_sigmas gpu={e_gpu:.3e} float32 cpu={e32:.3e} (max |reference| "
          f"{float(ref.abs().max()):.3e})")
    assert bool(torch.isfinite(sg.grad).all()) and float(ref.abs().max()) > 0
    assert e_gpu <= 4.0 * e32, (e_gpu, e32)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [5, 192])
def test_the_class(S):
    """the scalar equals the reference's sum over the counted pairs / their number, with and without the opacity mask
    and for patches that sit behind other rays (first_ray); an all-masked call returns 0 with gradients bitwise 0.
    Measured on the MI355X: values <= 1.2e-7, gradients <= 1.6e-7."""
    from fs_nerf_amd.core.loss import NeighborRayKLLoss
    case, g, fwd, cpu = _setup(S)
    R, ri, dev = case["R"], case["ri"], g["sig"].device
    bins, rng = 64, RANGES[0]
    edges = RH.edges_f32(bins, *rng)
    w64, t0, t1 = cpu["weights"].double(), case["t0"].double(), case["t1"].double()
    loss_fn = NeighborRayKLLoss(bins, t_min=rng[0], t_max=rng[1], threshold=THRESHOLD)
    c70 = cpu["opacity"].reshape(-1) > THRESHOLD
    for shape, first, masked in (((2, 5, 7), 0, False), ((2, 5, 7), 0, True), ((1, 6, 5), 33, True), ((3, 2, 4), 5, False)):
        n = shape[0] * shape[1] * shape[2]
        c = c70[first:first + n].reshape(shape) if masked else None
        w = fwd["weights"].detach().clone().requires_grad_(True)
        # (the mask from all 70 opacities or from the patch rays' own: both are accepted)
        op = None if not masked else (fwd["opacity"] if first % 2 else fwd["opacity"].reshape(-1)[first:first + n])
        loss = loss_fn(w, g["t0"], g["t1"], g["ri"], R, shape, first_ray=first, opacity=op)
        loss.backward()
        w_ref = w64.clone().requires_grad_(True)
        ref = RH.loss_value(w_ref, t0, t1, ri, R, edges, shape, first_ray=first, c=c)
        ref.backward()
        seven = ri == CR.ZERO_RAY
        ev = abs(float(loss.detach()) - float(ref.detach())) / abs(float(ref.detach()))
        eg = _rel(w.grad.cpu()[~seven], w_ref.grad[~seven])
        print(f"S={S} class {shape} first_ray={first} masked={masked}: value={ev:.3e} d_values={eg:.3e} "
              f"(pairs {RH.pair_count(c, shape)})")
        assert loss.shape == () and ev < TOL_FWD and eg < TOL_GRAD, (ev, eg)
        other = ((ri < first) | (ri >= first + n)).to(dev)
        assert _bits_zero(w.grad[other])
        if masked:
            off = (~c70)[ri].to(dev)
            assert _bits_zero(w.grad[off])
    w = fwd["weights"].detach().clone().requires_grad_(True)
    loss = loss_fn(w, g["t0"], g["t1"], g["ri"], R, (2, 5, 7), opacity=torch.zeros(R, 1, device=dev))
    loss.backward()
    assert float(loss.detach()) == 0.0 and _bits_zero(w.grad)
