#!/usr/bin/env python3
"""Time forward + backward of the neighbouring-ray KL (core.loss.NeighborRayKLLoss: csrc/ray_hist.hip) against the torch
spelling a user writes without the kernels: a broadcast overlap matrix [samples, bins] of min / max / clamp, index_add_
into the per-ray histograms (float atomics: not reproducible), slicing and log for the pairs.  The matrix is built in
chunks of samples when it would exceed --max-matrix-bytes (its temporaries are what the chunks bound; autograd keeps the
matrix itself either way).  Shapes: --patches 16 patches of --patch 16 x 16 rays with ragged spans (about --samples 150
samples per ray: a uniform count in [samples/2, 3 samples/2], every 64th ray empty - the input family of
tools/bench_ray_losses.py), --bins 64 over [2, 6], rays masked by opacity.  The timed call is loss + backward. Schedule:
interleaved (tools/benchlib.py), --rounds 3 rounds, us.  There is no pass or fail on these times.  Appends one JSON line
to profiles/bench_neighbor_kl.jsonl (--out) and prints it.

    timeout -k 10 300 python tools/bench_neighbor_kl.py [--iters 20] [--warmup 5] [--patches 16] [--patch 16] [--tag NAME]
"""
import argparse

import benchlib


def main():
    ap = argparse.ArgumentParser()
    benchlib.common_args(ap, iters=20, warmup=5, rounds=3, out="bench_neighbor_kl.jsonl")
    ap.add_argument("--patches", type=int, default=16)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=150)
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--max-matrix-bytes", type=int, default=1 << 30)
    args = ap.parse_args()
    import torch
    benchlib.package()
    from fs_nerf_amd import ops
    from fs_nerf_amd.core.loss import NeighborRayKLLoss
    dev = torch.device("cuda:0")
    B, Pp, S, bins = args.patches, args.patch, args.samples, args.bins
    R = B * Pp * Pp
    near, far = 2.0, 6.0
    gen = torch.Generator(device=dev).manual_seed(0)
    counts = torch.randint(S // 2, S + S // 2 + 1, (R,), device=dev, generator=gen)
    counts[::64] = 0
    ri = torch.repeat_interleave(torch.arange(R, device=dev), counts)
    N = ri.numel()
    first = torch.cumsum(counts, 0) - counts
    pos = (torch.arange(N, device=dev) - first[ri]).float()
    dt = (4.0 / counts.clamp(min=1).float())[ri]
    t0 = near + pos * dt
    t1 = t0 + dt
    sig = torch.rand(N, device=dev, generator=gen) * 3.0
    sig = torch.where(torch.rand(N, device=dev, generator=gen) < 0.05, -0.1 * sig, sig)
    rgb = torch.rand(N, 3, device=dev, generator=gen)
    _, opacity, _, ex = ops.composite_packed(sig, rgb, t0, t1, ri, R, [1.0, 1.0, 1.0])
    weights = ex["weights"].clone().requires_grad_(True)
    loss_fn = NeighborRayKLLoss(bins, t_min=near, t_max=far)
    edges = ops.ray_histogram_edges(bins, t_min=near, t_max=far).to(dev)
    chunk = max(1, min(N, args.max_matrix_bytes // (4 * bins)))

    def torch_loss():
        c = (opacity.detach().reshape(-1) > 0.1).reshape(B, Pp, Pp)
        ok = torch.isfinite(t0) & torch.isfinite(t1) & (t1 > t0)
        u = torch.where(ok, weights.clamp(min=0.0), torch.zeros_like(weights))
        H = torch.zeros(R, bins, device=dev)
        for a in range(0, N, chunk):
            s = slice(a, a + chunk)
            ov = (torch.minimum(t1[s, None], edges[None, 1:]) - torch.maximum(t0[s, None], edges[None, :-1])).clamp(min=0.0)
            f = torch.where(ok[s, None], ov / (t1[s] - t0[s])[:, None], torch.zeros_like(ov))
            H = H.index_add(0, ri[s], u[s, None] * f)
        P = (H / (torch.zeros(R, device=dev).index_add_(0, ri, u) + 1e-10)[:, None]).reshape(B, Pp, Pp, bins)
        lp = torch.log(P + 1e-5)
        right, down = c[:, :, :-1] & c[:, :, 1:], c[:, :-1] & c[:, 1:]
        dr = (P[:, :, :-1] * (lp[:, :, :-1] - lp[:, :, 1:])).sum(-1)
        dd = (P[:, :-1] * (lp[:, :-1] - lp[:, 1:])).sum(-1)
        total = torch.where(right, dr, torch.zeros_like(dr)).sum() + torch.where(down, dd, torch.zeros_like(dd)).sum()
        return total / (right.sum() + down.sum()).clamp(min=1)

    variants = {
        "neighbor_kl_kernel": lambda: loss_fn(weights, t0, t1, ri, R, (B, Pp, Pp), opacity=opacity),
        "neighbor_kl_torch": torch_loss,
    }
    a, b = (float(fn().detach()) for fn in variants.values())  # the two spellings compute the same loss
    agree = abs(a - b) / max(abs(b), 1e-12)
    rounds = benchlib.interleaved({name: (lambda fn=fn: torch.autograd.grad(fn(), weights)) for name, fn in variants.items()},
                                  args.iters, args.warmup, args.rounds)
    out = {**benchlib.header("bench_neighbor_kl", args.tag), "rays": R, "samples": N,
           "patches": [B, Pp, Pp], "bins": bins, "matrix_chunks": -(-N // chunk), "iters": args.iters, "rounds": args.rounds,
           "what": "loss forward + backward, device events, us", "loss": a,
           "relative_difference_of_the_two_spellings": agree,
           "variants": {name: benchlib.rounds_summary(r, "us") for name, r in rounds.items()}}
    benchlib.emit(out, args.out)


if __name__ == "__main__":
    main()
