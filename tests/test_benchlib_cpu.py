"""tools/benchlib.py without a GPU: the call order of the three schedules, what is dropped as warm-up, which statistic is
formed and what is appended to the record - driven by a fake clock that logs (variant, call number) and returns a
scripted value - and the shape of the ported tools/bench_*.py (no event pair, no appending open() of their own).
"""
import glob
import importlib.util
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
PORTED = ["bench_composite_bwd", "bench_depth_prior", "bench_fused", "bench_input_grad", "bench_intrinsics", "bench_invisible",
          "bench_loader", "bench_lpips", "bench_lpips_loss", "bench_march", "bench_metrics", "bench_mlp", "bench_neighbor_kl",
          "bench_occ_cone", "bench_pose_refine", "bench_propnet", "bench_ray_losses", "bench_refresh", "bench_ssim_loss",
          "bench_unseen", "bench_volrend", "bench_warp"]


@pytest.fixture()
def B(monkeypatch):
    spec = importlib.util.spec_from_file_location("benchlib", os.path.join(TOOLS, "benchlib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.log = []
    monkeypatch.setattr(mod, "synchronize", lambda: mod.log.append("sync"))
    return mod


def fake(B, script):
    """Variants a, b, c that log their own calls, and the clocks: sample k of variant v is script(v, k) (k counts that
    variant's calls from 0, the untimed warm-up calls of in_turns / windows included)."""
    n = {}

    def variant(v):
        def fn():
            n[v] = n.get(v, -1) + 1
            B.log.append((v, n[v]))
            return v
        return fn

    def clock(fn):
        v = fn()
        return script(v, n[v]), v

    def window_clock(fn, iters):
        v = fn()
        k = n[v]  # (the window's sample is scripted by the number of its first call)
        for _ in range(iters - 1):
            fn()
        return script(v, k)

    return {v: variant(v) for v in "abc"}, clock, window_clock


def value(v, k):
    return {"a": 100.0, "b": 200.0, "c": 300.0}[v] + [5.0, 9.0, 3.0, 1.0, 2.0][k % 5] + 10.0 * (k // 5)


def test_interleaved_order_warmup_and_medians(B):
    variants, clock, _ = fake(B, value)
    out = B.interleaved(variants, iters=3, warmup=2, rounds=2, clock=clock)
    assert [v for v, _ in B.log] == list("abc") * 10  # a b c five times per round, the two rounds one after the other
    assert list(out) == ["a", "b", "c"]
    # per round the samples are +5 +9 (dropped) +3 +1 +2 (kept: median +2), the second round 10 higher
    assert out == {"a": [102.0, 112.0], "b": [202.0, 212.0], "c": [302.0, 312.0]}


def test_interleaved_raw_samples(B):
    variants, clock, _ = fake(B, value)
    out = B.interleaved(variants, iters=3, warmup=2, rounds=1, keep="samples", clock=clock)
    assert out == {"a": [103.0, 101.0, 102.0], "b": [203.0, 201.0, 202.0], "c": [303.0, 301.0, 302.0]}
    with pytest.raises(AssertionError):
        B.interleaved(variants, iters=3, warmup=2, rounds=2, keep="samples", clock=clock)


def test_in_turns_order_and_medians(B):
    variants, clock, _ = fake(B, value)
    out = B.in_turns(variants, iters=3, warmup=2, rounds=2, clock=clock)
    one_round = []
    for v in "abc":
        one_round += [v] * 2 + ["sync"] + [v] * 3
    assert [e if e == "sync" else e[0] for e in B.log] == one_round * 2
    assert out == {"a": [102.0, 112.0], "b": [202.0, 212.0], "c": [302.0, 312.0]}
    B.log.clear()
    raw = B.in_turns({"a": variants["a"]}, iters=3, warmup=2, keep="samples", clock=clock)  # the single-variant form
    assert raw == {"a": [123.0, 121.0, 122.0]} and B.log.count("sync") == 1


def test_windows_order_and_window_length(B):
    variants, _, window_clock = fake(B, lambda v, k: float(k))
    out = B.windows(variants, iters=4, warmup=2, runs=3, clock=window_clock)
    order = [e if e == "sync" else e[0] for e in B.log]
    assert order[:7] == ["a", "a", "b", "b", "c", "c", "sync"]  # all warm-up calls first, then ONE synchronise
    assert order[7:] == (["a"] * 4 + ["b"] * 4 + ["c"] * 4) * 3 and "sync" not in order[7:]
    # every window starts where the last one of that variant ended: exactly `iters` calls each
    assert out == {"a": [2.0, 6.0, 10.0], "b": [2.0, 6.0, 10.0], "c": [2.0, 6.0, 10.0]}


def test_stats_and_rounds_summary(B):
    t = [0.123456, 0.5, 0.25, 1.0, 0.75, 0.3, 0.2, 0.9, 0.4, 0.6, 0.111111]
    assert B.stats(t) == {"median": 0.4, "min": 0.1111, "p90": 0.9}
    r = [0.26714249, 0.13976, 0.139644]  # ms, one per round
    # the spellings of profiles/bench_ray_losses.jsonl (us, 2 places) and profiles/bench_propnet.jsonl (ms, 4 places)
    assert B.rounds_summary(r, "us") == {"us_median": 139.76, "us_rounds": [267.14, 139.76, 139.64]}
    assert B.rounds_summary(r, "ms", per="runs") == {"ms_median": 0.1398, "ms_runs": [0.2671, 0.1398, 0.1396]}
    assert list(B.stats(t)) == ["median", "min", "p90"]  # profiles/bench_march.jsonl: "ms": {"median", "min", "p90"}


def test_emit_appends_one_line_per_call(B, tmp_path, capsys):
    out = tmp_path / "missing" / "dir" / "record.jsonl"
    B.emit({"tool": "t", "n": 1}, str(out))
    assert out.read_text() == '{"tool": "t", "n": 1}\n'
    B.emit({"tool": "t", "n": 2}, str(out))
    assert out.read_text() == '{"tool": "t", "n": 1}\n{"tool": "t", "n": 2}\n'
    before = sorted(p.name for p in tmp_path.rglob("*"))
    B.emit({"tool": "t", "n": 3})
    assert sorted(p.name for p in tmp_path.rglob("*")) == before and out.read_text().count("\n") == 2
    assert capsys.readouterr().out.splitlines() == ['{"tool": "t", "n": %d}' % n for n in (1, 2, 3)]


def test_run_child(B):
    env = dict(os.environ)
    with pytest.raises(SystemExit) as e:
        B.run_child([sys.executable, "-c", "import sys; print('said'); sys.exit(3)"], env, 30, "the failing child", "TAG ")
    assert "the failing child" in str(e.value) and "(3)" in str(e.value) and "said" in str(e.value)
    with pytest.raises(SystemExit) as e:
        B.run_child([sys.executable, "-c", "import time; time.sleep(30)"], env, 0.3, "the slow child", "TAG ")
    assert "the slow child" in str(e.value) and "limit" in str(e.value)
    got = B.run_child([sys.executable, "-c", "print('TAG {\"n\": 1}'); print('other'); print('TAG {\"n\": 2}'); print('end')"],
                      env, 30, "the good child", "TAG ")
    assert got == {"n": 2}


def test_common_args_adds_only_what_is_asked(B):
    import argparse
    ap = argparse.ArgumentParser()
    B.common_args(ap, iters=7, warmup=2, runs=4, out="x.jsonl")
    a = ap.parse_args([])
    assert (a.iters, a.warmup, a.runs, a.tag) == (7, 2, 4, "") and not hasattr(a, "rounds")
    assert a.out == os.path.join(ROOT, "profiles", "x.jsonl")
    ap = argparse.ArgumentParser()
    B.common_args(ap, iters=50, rounds=3, tag=False)
    assert vars(ap.parse_args([])) == {"iters": 50, "rounds": 3}


@pytest.mark.parametrize("tool", [t for t in PORTED if t != "bench_fused"])  # (bench_fused parses no arguments)
def test_help_exits_0_without_a_gpu(tool):
    r = subprocess.run([sys.executable, os.path.join(TOOLS, tool + ".py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    assert "--iters" in r.stdout or tool == "bench_mlp"


def test_no_tool_times_or_appends_by_itself():
    tools = sorted(glob.glob(os.path.join(TOOLS, "bench_*.py")))
    assert {os.path.basename(p)[:-3] for p in tools} >= set(PORTED)
    for path in tools:
        assert "torch.cuda.Event(" not in open(path).read(), path
    assert "torch.cuda.Event(" in open(os.path.join(TOOLS, "benchlib.py")).read()  # call_ms and window_ms: the only ones
    for tool in PORTED:
        text = open(os.path.join(TOOLS, tool + ".py")).read()
        assert not re.search(r"""open\([^)]*["']a["']""", text), tool
        assert "benchlib" in text, tool


def test_recorded_spellings_are_the_ones_checked_above():
    """The key names asserted in test_stats_and_rounds_summary are the ones the existing records hold."""
    def last(name):
        with open(os.path.join(ROOT, "profiles", name)) as fh:
            return json.loads(fh.read().splitlines()[-1])
    assert set(next(iter(last("bench_ray_losses.jsonl")["variants"].values()))) == {"us_median", "us_rounds"}
    assert set(last("bench_propnet.jsonl")["with_proposal_update"]) == {"ms_median", "ms_runs"}
    assert set(last("bench_march.jsonl")["uniform"]["ms"]) == {"median", "min", "p90"}
