#!/usr/bin/env python3
"""Cost of `DPVecEnv(reward_terms=True)` (dm_batch_imitation_terms, csrc/terms_kernel.h: one more launch per step) on one MI355X, written
as profiles/terms_kernels.md.  Three kinds of runs, the first two without a profiler:

  throughput    DPVecEnv.step env-steps/s (device tensors, one call's launches after the other's on one stream, a window closed by a
                device synchronise) with the option on and off, the two ALTERNATING in one process, `--reps` windows each (median and
                spread), at each `--envs` size of `walk` with the 5-term imitation reward and RSI auto-reset; every shape is warmed up.
  call time     the terms call alone, `--calls` of them back to back between two device events.
  kernel time   from `rocprofv3 --kernel-trace --stats` runs of their own (one per size), each running this file with `--trace N`: a few
                hundred steps with the option on, nothing timed.  Their `*_kernel_stats.csv` files come back through `--stats N=file`.

`--bench-lines file`: the default benchmark's JSON result lines of alternating runs of this commit and its parent, one per line, each
prefixed with `parent ` or `this `; the report lists their values and spreads.  `--float-notes file`: text recorded verbatim under
"float32" (the ratios the tests print).  `--resources-before file.md`: the table tools/kernel_resources.py printed for the library before
the kernel was added; the report says whether any pre-existing kernel changed.
usage: python tools/terms_bench.py [--envs 4096 8192] [--steps 200] [--warmup 30] [--reps 5] [--calls 2000] [--stats N=csv ...]
                                   [--bench-lines file] [--float-notes file] [--resources-before file.md] [--out profiles/terms_kernels.md]
       rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/terms_bench.py --trace 4096"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from state_bench import buffers, parse_before, read_stats, short      # noqa: E402  (the same measurement, another kernel)

HBM_PEAK = 8.0e12                                  # bytes/s, MI355X
BYTES_PER_ENV = (35 + 34 + 2 + 112 + 28) * 8       # qpos, qvel, the two cursors (counted as doubles), one table row (L2-resident after its first read), one output row
KERNEL = "k_imitation_terms"


def make_env(n, on):
    from deepmimic_mujoco_amd import DPVecEnv
    return DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, reward_terms=on)


def trace_run(n, steps, warmup):
    """the workload of a rocprofv3 run: `steps` closed-loop steps with the option on after `warmup`; nothing is timed here"""
    import torch
    dev = torch.device("cuda", 0)
    env = make_env(n, True)
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    out = buffers(n, 56, dev)
    env.reset("rsi")
    for _ in range(warmup + steps):
        env.step(ac, out=out)
    torch.cuda.synchronize()
    assert env.last_reward_terms.shape == (n, 28)
    env.close()
    print("trace run: %d envs, %d steps, packed=%s" % (n, warmup + steps, env.packed))


def measure(n, args):
    import torch
    dev = torch.device("cuda", 0)
    envs = {m: make_env(n, m == "on") for m in ("off", "on")}
    out = buffers(n, 56, dev)
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    rates = {m: [] for m in envs}
    for rep in range(args.reps):
        for m in ("off", "on") if rep % 2 == 0 else ("on", "off"):
            env = envs[m]
            env.reset("rsi")
            for _ in range(args.warmup):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            rates[m].append(n * args.steps / (time.perf_counter() - t0))
    b = envs["on"].batch
    rows = torch.zeros((n, 28), dtype=torch.float64, device=dev)
    for _ in range(50):
        b.imitation_terms(out=rows)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call_us = []
    for _ in range(3):
        e0.record()
        for _ in range(args.calls):
            b.imitation_terms(out=rows)
        e1.record(); e1.synchronize()
        call_us.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    assert bool(torch.isfinite(rows).all())
    res = dict(envs=n, packed=bool(envs["on"].packed), frame_skip=envs["on"].frame_skip)
    for m in envs:
        res[m] = dict(median=float(np.median(rates[m])), min=float(min(rates[m])), max=float(max(rates[m])))
        envs[m].close()
    res["ratio"] = res["on"]["median"] / res["off"]["median"]
    res["call_us"] = dict(median=float(np.median(call_us)), min=float(min(call_us)), max=float(max(call_us)))
    return res


def bench_section(path):
    L = ["## The default benchmark line with the option off (`bench.py --gpus 1`), this commit against its parent, alternating runs", ""]
    if not path or not os.path.exists(path):
        return L + ["not measured", ""]
    vals = {"parent": [], "this": []}
    L += ["| run | build | value | unit | spread of its windows (min / median / max) |", "|---|---|---|---|---|"]
    for i, ln in enumerate(x for x in open(path).read().splitlines() if x.strip()):
        tag, js = ln.split(" ", 1)
        r = json.loads(js)
        vals[tag].append(float(r["value"]))
        sp = r.get("value_spread") or {}
        L.append("| %d | %s | %.3f M | %s | %s |" % (i + 1, tag, r["value"] / 1e6, r.get("unit", ""), " / ".join("%.3f M" % (sp[k] / 1e6) for k in ("min", "median", "max") if k in sp)))
    if vals["parent"] and vals["this"]:
        mp, mt = float(np.median(vals["parent"])), float(np.median(vals["this"]))
        L += ["", "Median of the runs: parent %.3f M, this commit %.3f M (ratio %.4f); the parent's own runs span %.3f M .. %.3f M.  The step kernels' code objects are the"
              " parent's (resources below) and nothing is launched or allocated with the option off, so the line is the parent's by construction."
              % (mp / 1e6, mt / 1e6, mt / mp, min(vals["parent"]) / 1e6, max(vals["parent"]) / 1e6), ""]
    return L


def report(results, stats, args, device):
    L = ["# `DPVecEnv(reward_terms=True)`: cost of the imitation-terms kernel (`tools/terms_bench.py`)", "",
         "Device: %s.  `walk`, the 5-term imitation reward, RSI auto-reset, frame_skip %s, float64 library, device tensors, `DPVecEnv.step` calls back to back on one stream (a window"
         % (device, results[0]["frame_skip"] if results else "?"),
         "ends in a device synchronise).  Option on and off alternate in one process: %d windows of %d steps each after %d warm-up steps per window.  With the option on a step is the"
         % (args.reps, args.steps, args.warmup),
         "step launch, the terms launch and one masked fill (the NaN rows of the environments the step reset).", "",
         "## Throughput", "", "| envs | step kernel when the run ended | off env-steps/s (median, min .. max) | on env-steps/s (median, min .. max) | on / off |", "|---|---|---|---|---|"]
    if not results:
        L.append("| not measured | | | | |")
    for r in results:
        a, d = r["off"], r["on"]
        L.append("| %d | %s | %.3f M (%.3f .. %.3f) | %.3f M (%.3f .. %.3f) | %.4f |" % (r["envs"], "four envs per wave" if r["packed"] else "one env per wave", a["median"] / 1e6, a["min"] / 1e6,
                                                                                    a["max"] / 1e6, d["median"] / 1e6, d["min"] / 1e6, d["max"] / 1e6, r["ratio"]))
    L += ["", "## The terms call alone (device events around %d back-to-back calls, three windows)" % args.calls, "", "| envs | us per call (median, min .. max) |", "|---|---|"]
    if not results:
        L.append("| not measured | |")
    for r in results:
        c = r["call_us"]
        L.append("| %d | %.2f (%.2f .. %.2f) |" % (r["envs"], c["median"], c["min"], c["max"]))
    L += ["", "## Kernel time (`rocprofv3 --kernel-trace --stats`, a run of its own per size: `--trace N`)", "",
          "The expectation was `k_state_features`, the same shape of work (one wave per state around one `stage_kinematics` pass): 24.7 / 45.4 us at 4 096 / 8 192 envs (profiles/state_kernels.md).", ""]
    if not stats:
        L.append("not measured")
    for n, path in stats:
        rows = read_stats(path)
        tot = sum(r[3] for r in rows)
        k = [r for r in rows if KERNEL in r[0]]
        L += ["### %d envs" % n, ""]
        if k:
            ns = k[0][2]
            floor = n * BYTES_PER_ENV / HBM_PEAK
            L += ["`%s`: %.2f us per launch (%d launches), %.2f %% of the run's GPU kernel time.  Algorithmic bytes %d x %d = %.2f MB: at the HBM peak of %.0f TB/s that is "
                  "%.2f us, so the kernel runs at %.1f %% of HBM peak: like the features kernel it is bound by its kinematics pass and its LDS-limited residency, not by memory."
                  % (KERNEL, ns / 1e3, k[0][1], 100 * k[0][3] / tot, n, BYTES_PER_ENV, n * BYTES_PER_ENV / 1e6, HBM_PEAK / 1e12, floor * 1e6, 100 * floor / (ns * 1e-9)), ""]
        L += ["| kernel | launches | average us | share of GPU kernel time |", "|---|---|---|---|"]
        for r in rows[:8]:
            L.append("| %s | %d | %.2f | %.2f %% |" % (short(r[0]), r[1], r[2] / 1e3, 100 * r[3] / tot))
        L.append("")
    L += bench_section(args.bench_lines)
    L += ["## float32: the observed errors against the oracle-derived bars (tests/test_imitation_terms.py, tests/test_gpu_imitation_terms.py)", ""]
    L += [open(args.float_notes).read().rstrip(), ""] if args.float_notes and os.path.exists(args.float_notes) else ["not recorded", ""]
    import kernel_resources as KR
    L += ["## Resources (`tools/kernel_resources.py`: the code objects' own notes)", ""]
    tabs = {}
    for tag, lib in (("float64", "libdmenv.so"), ("float32", "libdmenv32.so")):
        tabs[tag] = KR.kernels(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", lib))
        for r in tabs[tag]:
            if KERNEL in r["name"]:
                L.append("`%s`, %s library: %d VGPR, %d SGPR, %d B LDS, %d B scratch, %d spilled: %d workgroups (= waves) per CU by LDS, %d waves per SIMD by registers."
                         % (KERNEL, tag, r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["vspill"] + r["sspill"], min(32, (160 * 1024) // r["lds"]), min(8, 512 // max(8, (r["vgpr"] + 7) // 8 * 8))))
    L += ["", "The kernel holds the step kernels' `Shared<Real>` (what `stage_kinematics` and `imitation_reward` work on) plus its 28-value row.", ""]
    if args.resources_before and os.path.exists(args.resources_before):
        was = parse_before(open(args.resources_before).read())
        now = {r["name"][:40]: (r["vgpr"], r["agpr"], r["sgpr"], r["vspill"], r["lds"], r["scratch"]) for r in tabs["float64"]}
        changed = sorted(k for k in was if k in now and was[k] != now[k]); gone = sorted(k for k in was if k not in now); new = sorted(k for k in now if k not in was)
        L += ["Before / after, float64 library (`imitation_reward` gained a defaulted template flag; the step kernels instantiate the old text): %d kernels before, %d after; new: %s; "
              "missing: %s; pre-existing kernels whose registers, LDS or scratch changed: %s." % (len(was), len(now), ", ".join(new) or "none", ", ".join(gone) or "none", ", ".join(changed) or "none"), ""]
    return "\n".join(L)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--trace", type=int, default=0, help="run only the workload of a rocprofv3 run at this many envs")
    ap.add_argument("--stats", nargs="*", default=[], help="N=path of a rocprofv3 kernel_stats.csv of a --trace N run")
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--float-notes", default=None)
    ap.add_argument("--resources-before", default=None)
    ap.add_argument("--results", default=None, help="read the throughput and call-time figures from this JSON (written by --json) instead of measuring")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terms_kernels.md"))
    ap.add_argument("--json", default=None, help="also write the raw figures here")
    args = ap.parse_args(argv)
    if args.trace:
        trace_run(args.trace, args.steps, args.warmup)
        return
    if args.results:
        saved = json.loads(open(args.results).read())
        results, device = saved["results"], saved["device"]
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("terms_bench.py measures on a GPU: none is visible")
        results, device = [measure(n, args) for n in args.envs], torch.cuda.get_device_name(0)
    stats = [(int(s.split("=", 1)[0]), s.split("=", 1)[1]) for s in args.stats]
    txt = report(results, stats, args, device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    if args.json:
        open(args.json, "w").write(json.dumps(dict(results=results, device=device)) + "\n")
    print(txt)


if __name__ == "__main__":
    main()
