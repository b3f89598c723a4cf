#!/usr/bin/env python3
"""Cost of `obs_mode="deepmimic"` (dm_batch_state_features, csrc/state_kernel.h: one more launch per step) on one MI355X, written as
profiles/state_kernels.md.  Three kinds of runs, the first two without a profiler:

  throughput    DPVecEnv.step env-steps/s (device tensors, one call's launches after the other's on one stream, a window closed by a
                device synchronise) with each observation
                mode, the two ALTERNATING in one process, `--reps` windows each (median and spread), at each `--envs` size of `walk` with
                the 5-term imitation reward and RSI auto-reset; every shape is warmed up first.
  call time     the features call alone, `--calls` of them back to back between two device events.
  kernel time   from `rocprofv3 --kernel-trace --stats` runs of their own (one per size), each running this file with `--trace N`: a few
                hundred "deepmimic" steps, nothing timed.  Their `*_kernel_stats.csv` files come back through `--stats N=file`; the
                report then states the features kernel's time, its share of HBM peak from its algorithmic bytes
                ((35 + 34 + 2 + 171) * 8 per environment) and where a step's GPU time goes.

`--resources-before file.md`: the table tools/kernel_resources.py printed for the library BEFORE the features kernel was added; the
report lists it next to the current one and says whether any pre-existing kernel changed.
usage: python tools/state_bench.py [--envs 4096 8192] [--steps 200] [--warmup 30] [--reps 5] [--calls 2000] [--stats N=csv ...]
                                   [--resources-before file.md] [--out profiles/state_kernels.md]
       rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/state_bench.py --trace 4096"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12                                  # bytes/s, MI355X
BYTES_PER_ENV = (35 + 34 + 2 + 171) * 8            # qpos, qvel, the two cursor fields (counted as doubles), one output row


def make_env(n, obs_mode):
    from deepmimic_mujoco_amd import DPVecEnv
    return DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, obs_mode=obs_mode)


def buffers(n, width, dev):
    import torch
    return (torch.zeros((n, width), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))


def trace_run(n, steps, warmup):
    """the workload of a rocprofv3 run: `steps` closed-loop "deepmimic" steps after `warmup`; nothing is timed here"""
    import torch
    dev = torch.device("cuda", 0)
    env = make_env(n, "deepmimic")
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    out = buffers(n, 171, dev)
    env.reset("rsi")
    for _ in range(warmup + steps):
        env.step(ac, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all())
    env.close()
    print("trace run: %d envs, %d steps, packed=%s" % (n, warmup + steps, env.packed))


def measure(n, args):
    import torch
    dev = torch.device("cuda", 0)
    envs = {m: make_env(n, m) for m in ("dp_env_v3", "deepmimic")}
    outs = {"dp_env_v3": buffers(n, 56, dev), "deepmimic": buffers(n, 171, dev)}
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    rates = {m: [] for m in envs}
    for rep in range(args.reps):
        for m in ("dp_env_v3", "deepmimic") if rep % 2 == 0 else ("deepmimic", "dp_env_v3"):
            env, out = envs[m], outs[m]
            env.reset("rsi")
            for _ in range(args.warmup):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            rates[m].append(n * args.steps / (time.perf_counter() - t0))
    # the features call alone, device events around `calls` of them
    b = envs["deepmimic"].batch
    feat = outs["deepmimic"][0]
    for _ in range(50):
        b.state_features(feat)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    call_us = []
    for _ in range(3):
        e0.record()
        for _ in range(args.calls):
            b.state_features(feat)
        e1.record(); e1.synchronize()
        call_us.append(e0.elapsed_time(e1) * 1e3 / args.calls)
    assert bool(torch.isfinite(feat).all())
    res = dict(envs=n, packed=bool(envs["deepmimic"].packed), frame_skip=envs["deepmimic"].frame_skip)
    for m in envs:
        res[m] = dict(median=float(np.median(rates[m])), min=float(min(rates[m])), max=float(max(rates[m])))
        envs[m].close()
    res["ratio"] = res["deepmimic"]["median"] / res["dp_env_v3"]["median"]
    res["call_us"] = dict(median=float(np.median(call_us)), min=float(min(call_us)), max=float(max(call_us)))
    return res


def read_stats(path):
    """rows of a rocprofv3 kernel_stats.csv -> [(name, calls, average ns, total ns)] by descending total"""
    rows = []
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        rows.append((name, int(float(r["Calls"])), float(r["AverageNs"]), float(r["TotalDurationNs"])))
    return sorted(rows, key=lambda r: -r[3])


def short(name):
    return name.split("(")[0].replace("void ", "")[:48]


def resources_tables(before_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    out = {}
    for tag, lib in (("float64", "libdmenv.so"), ("float32", "libdmenv32.so")):
        rows = sorted(KR.kernels(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", lib)), key=lambda r: (-r["vgpr"], r["name"]))
        out[tag] = rows
    before = open(before_path).read() if before_path and os.path.exists(before_path) else None
    return out, before


def fmt_rows(rows):
    lines = ["| kernel | VGPR | of which AGPR | SGPR | spilled VGPR | LDS B | scratch B/lane | waves/SIMD by registers | workgroups/CU by LDS |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        regs = 512 // max(8, (r["vgpr"] + 7) // 8 * 8) if r["vgpr"] else 8
        lds = (160 * 1024) // r["lds"] if r["lds"] else 32
        lines.append("| %s | %d | %d | %d | %d | %d | %d | %d | %d |" % (r["name"][:40], r["vgpr"], r["agpr"], r["sgpr"], r["vspill"], r["lds"], r["scratch"], min(8, regs), min(32, lds)))
    return lines


def parse_before(txt):
    """{kernel: (vgpr, agpr, sgpr, spilled vgpr, lds, scratch)} from a tools/kernel_resources.py table"""
    out = {}
    for ln in txt.splitlines():
        c = [x.strip() for x in ln.strip().strip("|").split("|")]
        if len(c) >= 8 and c[1].isdigit():
            out[c[0]] = (int(c[1]), int(c[2]), int(c[3]), int(c[4]), int(c[6]), int(c[7]))
    return out


def report(results, stats, args, device):
    L = ["# `obs_mode=\"deepmimic\"`: cost of the state-features kernel (`tools/state_bench.py`)", "",
         "Device: %s.  `walk`, the 5-term imitation reward, RSI auto-reset, frame_skip %s, float64 library, device tensors, `DPVecEnv.step` calls back to back on one stream (a window"
         % (device, results[0]["frame_skip"] if results else "?"),
         "ends in a device synchronise).  Both observation modes alternate in one process: %d windows of %d steps each after %d warm-up steps per window."
         % (args.reps, args.steps, args.warmup), "",
         "## Throughput", "", "| envs | step kernel when the run ended (the batch re-decides every 256 steps) | dp_env_v3 env-steps/s (median, min .. max) | deepmimic env-steps/s (median, min .. max) | deepmimic / dp_env_v3 |", "|---|---|---|---|---|"]
    if not results:
        L.append("| not measured | | | | |")
    for r in results:
        a, d = r["dp_env_v3"], r["deepmimic"]
        L.append("| %d | %s | %.3f M (%.3f .. %.3f) | %.3f M (%.3f .. %.3f) | %.4f |" % (r["envs"], "four envs per wave" if r["packed"] else "one env per wave", a["median"] / 1e6, a["min"] / 1e6,
                                                                                    a["max"] / 1e6, d["median"] / 1e6, d["min"] / 1e6, d["max"] / 1e6, r["ratio"]))
    for r in results:
        tr = [read_stats(path) for n, path in stats if n == r["envs"]]
        feat = [x for x in tr[0] if "k_state_features" in x[0]] if tr else []
        if feat:
            L += ["", "%d envs: the \"deepmimic\" rate is %.2f %% below the default's; in the trace below the features kernel is %.2f %% of a step's GPU kernel time, which accounts for it"
                  " (the trace's steps are a run's first ones: the kernel the batch starts on)." % (r["envs"], 100 * (1 - r["ratio"]), 100 * feat[0][3] / sum(x[3] for x in tr[0]))]
    L += ["", "## The features call alone (device events around %d back-to-back calls, three windows)" % args.calls, "", "| envs | us per call (median, min .. max) |", "|---|---|"]
    if not results:
        L.append("| not measured | |")
    for r in results:
        c = r["call_us"]
        L.append("| %d | %.2f (%.2f .. %.2f) |" % (r["envs"], c["median"], c["min"], c["max"]))
    L += ["", "## Kernel time (`rocprofv3 --kernel-trace --stats`, a run of its own per size: `--trace N`)", ""]
    if not stats:
        L.append("not measured")
    for n, path in stats:
        rows = read_stats(path)
        tot = sum(r[3] for r in rows)
        feat = [r for r in rows if "k_state_features" in r[0]]
        L += ["### %d envs" % n, ""]
        if feat:
            ns = feat[0][2]
            floor = n * BYTES_PER_ENV / HBM_PEAK
            L += ["`k_state_features`: %.2f us per launch (%d launches), %.2f %% of the run's GPU kernel time.  Algorithmic bytes %d x %d = %.2f MB: at the HBM peak of %.0f TB/s that is "
                  "%.2f us, so the kernel runs at %.1f %% of HBM peak (%.2f TB/s)."
                  % (ns / 1e3, feat[0][1], 100 * feat[0][3] / tot, n, BYTES_PER_ENV, n * BYTES_PER_ENV / 1e6, HBM_PEAK / 1e12, floor * 1e6, 100 * floor / (ns * 1e-9),
                     n * BYTES_PER_ENV / (ns * 1e-9) / 1e12), ""]
        L += ["| kernel | launches | average us | share of GPU kernel time |", "|---|---|---|---|"]
        for r in rows[:8]:
            L.append("| %s | %d | %.2f | %.2f %% |" % (short(r[0]), r[1], r[2] / 1e3, 100 * r[3] / tot))
        L.append("")
    tabs, before = resources_tables(args.resources_before)
    L += ["## Resources (`tools/kernel_resources.py`: the code objects' own notes)", ""]
    for tag in ("float64", "float32"):
        f = [r for r in tabs[tag] if "k_state_features" in r["name"]]
        if f:
            r = f[0]
            L.append("`k_state_features`, %s library: %d VGPR, %d SGPR, %d B LDS, %d B scratch, no spills: %d workgroups (= waves) per CU by LDS, %d waves per SIMD by registers."
                     % (tag, r["vgpr"], r["sgpr"], r["lds"], r["scratch"], min(32, (160 * 1024) // r["lds"]), min(8, 512 // max(8, (r["vgpr"] + 7) // 8 * 8))))
    L += ["", "The kernel holds the step kernels' `Shared<Real>` (what `stage_kinematics` works on) plus its 171-value row.", ""]
    f64 = [r for r in tabs["float64"] if "k_state_features" in r["name"]]
    if f64 and stats:
        by_lds, by_reg = min(32, (160 * 1024) // f64[0]["lds"]), 4 * min(8, 512 // max(8, (f64[0]["vgpr"] + 7) // 8 * 8))
        L += ["### Occupancy: would a smaller LDS struct, or several environments per wave, pay?", "",
              "One wave per environment; a kinematics pass keeps 13 to 34 of its 64 lanes busy.  LDS bounds the residency at %d waves per CU (x 256 CUs = %d resident waves)"
              % (by_lds, 256 * by_lds),
              "where the registers would allow %d.  A struct holding only what the features read (qpos, qvel, xpos, xquat, xmat, xipos, the dof axes, the row: about 5 KB in float64)"
              % by_reg,
              "would lift the LDS bound above the register bound; it needs a kinematics routine of its own, because the step kernels' `stage_kinematics` takes `Shared<Real>&`",
              "and also fills the spatial inertias there.  What that could buy is bounded by the kernel's measured time:", ""]
        for n, path in stats:
            rows = read_stats(path)
            feat = [r for r in rows if "k_state_features" in r[0]]
            if not feat:
                continue
            calls = feat[0][1]
            per_step = sum(r[3] for r in rows) / calls
            rounds = -(-n // (256 * by_lds))
            L.append("- %d envs: %d waves in %d round(s) of the LDS-bound residency; the kernel takes %.2f us of the %.1f us of GPU kernel time per step (%.2f %%).  Even a kernel"
                     " twice as fast would save %.2f us per step, %.2f %% of it." % (n, n, rounds, feat[0][2] / 1e3, per_step / 1e3, 100 * feat[0][2] / per_step,
                                                                                    feat[0][2] / 2e3, 50 * feat[0][2] / per_step))
        L += ["", "The kernel's time grows with the number of rounds (compare the sizes above), so doubling the residency is what could come close to halving it.",
              "Not built: the saving is bounded as above, and a second kinematics routine would have to be kept equal to the one every other kernel shares.", ""]
    if before:
        was = parse_before(before)
        now = {r["name"][:40]: (r["vgpr"], r["agpr"], r["sgpr"], r["vspill"], r["lds"], r["scratch"]) for r in tabs["float64"]}
        changed = sorted(k for k in was if k in now and was[k] != now[k]); gone = sorted(k for k in was if k not in now); new = sorted(k for k in now if k not in was)
        L += ["Before / after, float64 library: %d kernels before, %d after; new: %s; missing: %s; pre-existing kernels whose registers, LDS or scratch changed: %s."
              % (len(was), len(now), ", ".join(new) or "none", ", ".join(gone) or "none", ", ".join(changed) or "none"), "", "### Before (float64 library)", ""]
        L += [ln for ln in before.splitlines() if ln.startswith("|")]
        L.append("")
    L += ["### After (float64 library)", ""] + fmt_rows(tabs["float64"]) + ["", "### After (float32 library)", ""] + fmt_rows(tabs["float32"]) + [""]
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
    ap.add_argument("--resources-before", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "state_kernels.md"))
    ap.add_argument("--json", default=None, help="also write the raw figures here")
    args = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("state_bench.py measures on a GPU: none is visible")
    if args.trace:
        trace_run(args.trace, args.steps, args.warmup)
        return
    results = [measure(n, args) for n in args.envs]
    stats = [(int(s.split("=", 1)[0]), s.split("=", 1)[1]) for s in args.stats]
    txt = report(results, stats, args, torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt)
    if args.json:
        open(args.json, "w").write(json.dumps(results) + "\n")
    print(txt)


if __name__ == "__main__":
    main()
