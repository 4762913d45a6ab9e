"""The one place where the tools/bench_*.py feature benchmarks time, summarise and record.

All times are CALL times in ms from two device events around a call, the host launch path included.  Three schedules
turn `variants` (dict name -> callable, called in that order) into dict name -> list of samples:

  interleaved  every variant once per iteration, warm-up iterations dropped; per round the median of the kept samples
  in_turns     per round each variant by itself: warm-up, a synchronise, `iters` timed calls; one median per round
  windows      every variant's warm-up once, one synchronise, then per run ONE event pair around `iters` calls

There is no CPU mode: without a GPU the first event fails.  `clock` is there for tests/test_benchlib_cpu.py alone.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def package(root=ROOT):
    """Put the checkout `root` in front of sys.path and import its package; -> root."""
    root = os.path.abspath(root)
    sys.path.insert(0, root)
    import fs_nerf_amd  # noqa: F401
    return root


def synchronize():
    import torch
    torch.cuda.synchronize()


def call_ms(fn):
    """-> (ms, fn()): one call between two device events; nothing else sits between the two records."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def window_ms(fn, iters):
    """-> ms per call over one window of `iters` back-to-back calls between two device events."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _kept(times, keep):
    return times if keep == "samples" else [float(np.median(times))]


def interleaved(variants, iters, warmup, rounds=1, keep="medians", clock=call_ms):
    """The variants alternate call by call, so that clock and thermal drift hit all alike.  keep="samples" (one round
    only) returns the raw kept samples instead of their median."""
    assert keep == "medians" or rounds == 1
    out = {name: [] for name in variants}
    for _ in range(rounds):
        times = {name: [] for name in variants}
        for it in range(warmup + iters):
            for name, fn in variants.items():
                ms = clock(fn)[0]
                if it >= warmup:
                    times[name].append(ms)
        for name in variants:
            out[name] += _kept(times[name], keep)
    return out


def in_turns(variants, iters, warmup, rounds=1, keep="medians", clock=call_ms):
    """The variants take turns inside every round, each with a warm-up of its own.  keep as in `interleaved`."""
    assert keep == "medians" or rounds == 1
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            for _ in range(warmup):
                fn()
            synchronize()
            out[name] += _kept([clock(fn)[0] for _ in range(iters)], keep)
    return out


def windows(variants, iters, warmup, runs, clock=window_ms):
    """All warm-ups first, then the variants alternate run by run, one window of `iters` calls each."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    synchronize()
    out = {name: [] for name in variants}
    for _ in range(runs):
        for name, fn in variants.items():
            out[name].append(clock(fn, iters))
    return out


def stats(samples):
    return {"median": round(float(np.median(samples)), 4), "min": round(float(np.min(samples)), 4),
            "p90": round(float(np.percentile(samples, 90)), 4)}


def rounds_summary(samples, unit, per="rounds"):
    """ms samples, one per round (or run) -> {"<unit>_median", "<unit>_<per>"}: us to 2 places, ms to 4."""
    scale, places = {"us": (1e3, 2), "ms": (1.0, 4)}[unit]
    return {f"{unit}_median": round(float(np.median(samples)) * scale, places),
            f"{unit}_{per}": [round(x * scale, places) for x in samples]}


def common_args(ap, *, iters, warmup=None, rounds=None, runs=None, tag=True, out=None):
    """Add the shared flags a tool has, with that tool's defaults; `out` names its record under profiles/."""
    ap.add_argument("--iters", type=int, default=iters)
    for flag, default in (("--warmup", warmup), ("--rounds", rounds), ("--runs", runs)):
        if default is not None:
            ap.add_argument(flag, type=int, default=default)
    if tag:
        ap.add_argument("--tag", default="")
    if out:
        ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))


def header(tool, tag):
    import torch
    return {"tool": tool, "tag": tag, "device": torch.cuda.get_device_name(0)}


def emit(line, out=None):
    """Print the record as one JSON line; with `out`, append it to that file (its directory is made)."""
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(text + "\n")


def run_child(cmd, env, limit, who, tag, cwd=ROOT):
    """One child process under a time limit of its own -> the JSON behind its last line that starts with `tag`.
    A timeout or a non-zero exit raises SystemExit, so that nothing more is started on the GPU afterwards."""
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=cwd, timeout=limit)
    except subprocess.TimeoutExpired as e:
        tails = "".join((s.decode(errors="replace") if isinstance(s, bytes) else s or "")[-2000:] for s in (e.stdout, e.stderr))
        raise SystemExit(f"{who} ran past its {limit} s limit; stopping\n" + tails)
    if r.returncode != 0:
        raise SystemExit(f"{who} failed ({r.returncode}); stopping\n" + r.stdout[-2000:] + r.stderr[-3000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith(tag)][-1][len(tag):])
