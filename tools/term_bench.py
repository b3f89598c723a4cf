#!/usr/bin/env python3
"""Cost of early termination (DM_OPT_FALL_BODIES, csrc/term_kernel.h: one more launch per step) on one MI355X, written as
profiles/term_kernels.md.  Modelled on tools/state_bench.py; two kinds of runs, the first without a profiler:

  throughput    DPVecEnv.step env-steps/s (device tensors, one call's launches after the other's on one stream, a window closed by a device
                synchronise) with termination off and with the "deepmimic" fall set, the two ALTERNATING in one process, `--reps` windows
                each (median and spread), at each `--envs` size of `walk` with the 5-term imitation reward and RSI auto-reset; every shape is
                warmed up first.  The off leg issues exactly the launches of a build without the feature.
  kernel time   from `rocprofv3 --kernel-trace --stats` runs of their own (one per size), each running this file with `--trace N`: a few
                hundred steps with termination on, nothing timed.  Their `*_kernel_stats.csv` files come back through `--stats N=file`; the
                report then states k_terminate's time per launch and where a step's GPU time goes.

`--truncation-log`: the cost of the truncation log (DM_OPT_TRUNCATION_LOG: one atomic and 73 stores per environment the time limit truncates) instead:
the same two kinds of runs with the time limit on (`--limit` env steps; after the window's RSI reset every environment reaches it on the same step, the
worst case for the log) and the log off / on alternating; `--trace N --truncation-log` is the profiled workload.  The report is APPENDED to `--out` as a
section of its own.

`--resources-before file.md`: the table tools/kernel_resources.py printed for the library BEFORE the feature; the report lists the step
kernels' rows of both and says whether any pre-existing kernel changed.  `--ab file`: the alternating parent / this-build lines of the
default benchmark (tools/ab_bench.sh's form), quoted in the report.
`--horizon`: DM_OPT_HORIZON_TERMINATION (termination inside the horizon launch) off against on, and against the horizon launch without termination: one
fused-policy dm_batch_rollout per window, the legs alternating in one process; one JSON line per size (profiles/term_horizon.md quotes them).
usage: python tools/term_bench.py --horizon [--envs 4096 8192] [--steps 128] [--reps 5]
       python tools/term_bench.py --truncation-log [--limit 10] [--envs 4096 8192] [--stats N=csv ...] [--resources-before file.md] [--train-json file]
       python tools/term_bench.py [--envs 4096 8192] [--steps 200] [--warmup 30] [--reps 5] [--stats N=csv ...] [--resources-before file.md]
                                  [--ab file] [--out profiles/term_kernels.md]
       rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/term_bench.py --trace 4096"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from state_bench import buffers, parse_before, read_stats, short  # noqa: E402


def make_env(n, fall, limit=0, log=0):
    from deepmimic_mujoco_amd import DPVecEnv
    return DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, fall_contact_bodies=fall, max_episode_steps=limit, truncation_log=log)


def log_capacity(n, args):
    """records a window can produce: every environment once per `--limit` steps, warm-up included (the log is cleared before every window)"""
    return n * ((args.warmup + args.steps) // args.limit + 1)


def trace_run(n, steps, warmup, args=None):
    """the workload of a rocprofv3 run: closed-loop steps with the "deepmimic" fall set (--truncation-log: with the time limit and the log); nothing is timed here"""
    import torch
    dev = torch.device("cuda", 0)
    env = make_env(n, None, args.limit, log_capacity(n, args)) if args is not None and args.truncation_log else make_env(n, "deepmimic")
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    out = buffers(n, 56, dev)
    env.reset("rsi")
    for _ in range(warmup + steps):
        env.step(ac, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[0]).all())
    print("trace run: %d envs, %d steps, packed=%s" % (n, warmup + steps, env.packed))
    env.close()


def measure(n, args):
    import torch
    from deepmimic_mujoco_amd import _abi as A
    dev = torch.device("cuda", 0)
    if args.truncation_log:
        envs = {"off": make_env(n, None, args.limit), "on": make_env(n, None, args.limit, log_capacity(n, args))}
    else:
        envs = {"off": make_env(n, None), "on": make_env(n, "deepmimic")}
    out = buffers(n, 56, dev)
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    rates = {m: [] for m in envs}
    ended = {m: 0 for m in envs}
    logged = 0
    for rep in range(args.reps):
        for m in ("off", "on") if rep % 2 == 0 else ("on", "off"):
            env = envs[m]
            env.reset("rsi")
            if args.truncation_log and m == "on":
                env.truncations(clear=True)
            for _ in range(args.warmup):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            ep0 = int(env.batch.get(A.F_EPISODE).sum())
            t0 = time.perf_counter()
            for _ in range(args.steps):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            rates[m].append(n * args.steps / (time.perf_counter() - t0))
            ended[m] += int(env.batch.get(A.F_EPISODE).sum()) - ep0
            if args.truncation_log and m == "on":
                cnt = int(env.truncations(clear=False)[0][0])
                assert 0 < cnt <= log_capacity(n, args), "the log overflowed or stayed empty: %d" % cnt
                logged = logged + cnt if rep else cnt
    res = dict(envs=n, packed=bool(envs["on"].packed), frame_skip=envs["on"].frame_skip)
    for m in envs:
        res[m] = dict(median=float(np.median(rates[m])), min=float(min(rates[m])), max=float(max(rates[m])), episodes=ended[m])
        envs[m].close()
    res["ratio"] = res["on"]["median"] / res["off"]["median"]
    if args.truncation_log:
        res["records"] = logged
    return res


def report_log(results, stats, args, device):
    """the section `--truncation-log` appends to the report"""
    L = ["", "# The truncation log: cost of `DM_OPT_TRUNCATION_LOG` (`tools/term_bench.py --truncation-log`)", "",
         "Device: %s.  The workload of the sections above with `max_episode_steps=%d` and no fall set; the log off and on (capacity: every environment once per %d steps of a"
         % (device, args.limit, args.limit),
         "window, cleared before each) alternate in one process, %d windows of %d steps after %d warm-up steps.  Every window starts from an RSI reset of the whole batch, so all"
         % (args.reps, args.steps, args.warmup),
         "environments that the step does not end itself reach the limit on the same step: the log's worst case (one atomic on one counter and 73 stores per truncating environment).", "",
         "| envs | step kernel when the run ended | log off env-steps/s (median, min .. max) | log on env-steps/s (median, min .. max) | on / off | records logged in the windows |",
         "|---|---|---|---|---|---|"]
    for r in results:
        a, d = r["off"], r["on"]
        L.append("| %d | %s | %.3f M (%.3f .. %.3f) | %.3f M (%.3f .. %.3f) | %.4f | %d |"
                 % (r["envs"], "four envs per wave" if r["packed"] else "one env per wave", a["median"] / 1e6, a["min"] / 1e6, a["max"] / 1e6, d["median"] / 1e6, d["min"] / 1e6,
                    d["max"] / 1e6, r["ratio"], r.get("records", 0)))
    L += ["", "## `k_terminate` with the log on (`rocprofv3 --kernel-trace --stats`, a run of its own: `--trace N --truncation-log`)", ""]
    if not stats:
        L.append("not measured")
    for n, path in stats:
        rows = read_stats(path)
        tot = sum(r[3] for r in rows)
        term = [r for r in rows if "k_terminate" in r[0]]
        if term:
            L += ["%d envs: `k_terminate` %.2f us per launch (%d launches), %.2f %% of the run's GPU kernel time." % (n, term[0][2] / 1e3, term[0][1], 100 * term[0][3] / tot), ""]
    if args.train_json and os.path.exists(args.train_json):
        L += ["## Training (`tools/train_trpo.py`, 4 096 envs x 128 steps, `--max-episode-steps 600`, with and without `--bootstrap-time-limit`, alternating)", "", "```"]
        L += [ln.rstrip() for ln in open(args.train_json).read().splitlines() if ln.strip()]
        L += ["```", ""]
    rows, before = resources(args.resources_before)
    if "k_terminate" in rows:
        r = rows["k_terminate"]
        L += ["## Resources", "", "`k_terminate`: %d VGPR, %d SGPR, %d B LDS, %d B scratch, %d spilled VGPR." % (r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["vspill"]), ""]
    if before is not None:
        now = {k: (r["vgpr"], r["agpr"], r["sgpr"], r["vspill"], r["lds"], r["scratch"]) for k, r in rows.items()}
        changed = sorted(k for k in before if k in now and now[k] != before[k])
        L += ["Against the table of the library before the log: %d kernels then, %d now; new: %s; pre-existing kernels whose row changed: %s."
              % (len(before), len(now), ", ".join("`%s`" % k for k in sorted(k for k in now if k not in before)) or "none", ", ".join("`%s`" % k for k in changed) or "none"), ""]
    return "\n".join(L) + "\n"


def resources(before_path):
    import kernel_resources as KR
    rows = {r["name"]: r for r in KR.kernels(os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "libdmenv.so"))}
    before = parse_before(open(before_path).read()) if before_path and os.path.exists(before_path) else None
    return rows, before


def report(results, stats, args, device):
    L = ["# Early termination: cost of the termination launch (`tools/term_bench.py`)", "",
         "Device: %s.  `walk`, the 5-term imitation reward, RSI auto-reset, frame_skip %s, float64 library, device tensors, `DPVecEnv.step` calls back to back on one stream"
         % (device, results[0]["frame_skip"] if results else "?"),
         "(a window ends in a device synchronise).  Termination off and `fall_contact_bodies=\"deepmimic\"` alternate in one process: %d windows of %d steps each after %d warm-up"
         % (args.reps, args.steps, args.warmup),
         "steps per window.  The off leg issues the launches of a build without the feature.", "",
         "## Throughput", "", "| envs | step kernel when the run ended | off env-steps/s (median, min .. max) | on env-steps/s (median, min .. max) | on / off | episodes ended in the windows, off / on |",
         "|---|---|---|---|---|---|"]
    if not results:
        L.append("| not measured | | | | | |")
    for r in results:
        a, d = r["off"], r["on"]
        L.append("| %d | %s | %.3f M (%.3f .. %.3f) | %.3f M (%.3f .. %.3f) | %.4f | %d / %d |"
                 % (r["envs"], "four envs per wave" if r["packed"] else "one env per wave", a["median"] / 1e6, a["min"] / 1e6, a["max"] / 1e6, d["median"] / 1e6, d["min"] / 1e6,
                    d["max"] / 1e6, r["ratio"], a["episodes"], d["episodes"]))
    L += ["", "With the fall set on, episodes may end earlier, and an environment early in its episode is a different workload from a late one: the ratio is the cost of the launch",
          "plus that shift.  The kernel's own time is below.", "",
          "## Kernel time (`rocprofv3 --kernel-trace --stats`, a run of its own per size: `--trace N`)", ""]
    if not stats:
        L.append("not measured")
    for n, path in stats:
        rows = read_stats(path)
        tot = sum(r[3] for r in rows)
        term = [r for r in rows if "k_terminate" in r[0]]
        L += ["### %d envs" % n, ""]
        if term:
            L += ["`k_terminate`: %.2f us per launch (%d launches), %.2f %% of the run's GPU kernel time.  (For scale: the state-features launch, the same shape — kinematics plus a light"
                  " epilogue — is 2.7-2.8 %% of a step, profiles/state_kernels.md.)" % (term[0][2] / 1e3, term[0][1], 100 * term[0][3] / tot), ""]
        L += ["| kernel | launches | average us | share of GPU kernel time |", "|---|---|---|---|"]
        for r in rows[:8]:
            L.append("| %s | %d | %.2f | %.2f %% |" % (short(r[0]), r[1], r[2] / 1e3, 100 * r[3] / tot))
        L.append("")
    if args.ab and os.path.exists(args.ab):
        L += ["## The default benchmark line, parent build against this one (alternating runs in one process chain, the form of `tools/ab_bench.sh`)", "", "```"]
        L += [ln.rstrip() for ln in open(args.ab).read().splitlines() if ln.strip()]
        L += ["```", ""]
    rows, before = resources(args.resources_before)
    L += ["## Resources (`tools/kernel_resources.py`: the code objects' own notes)", ""]
    for k in ("k_terminate", "k_floor_contacts"):
        if k in rows:
            r = rows[k]
            L.append("`%s`: %d VGPR, %d SGPR, %d B LDS, %d B scratch, %d spilled VGPR." % (k, r["vgpr"], r["sgpr"], r["lds"], r["scratch"], r["vspill"]))
    L.append("")
    if before is None:
        L.append("No table of the library before the feature was given (`--resources-before`).")
    else:
        now = {k: (r["vgpr"], r["agpr"], r["sgpr"], r["vspill"], r["lds"], r["scratch"]) for k, r in rows.items()}
        changed = sorted(k for k in before if k in now and now[k] != before[k])
        gone = sorted(k for k in before if k not in now)
        new = sorted(k for k in now if k not in before)
        L += ["Against the table of the library before the feature: %d kernels then, %d now; new: %s; removed: %s; pre-existing kernels whose row changed: %s."
              % (len(before), len(now), ", ".join("`%s`" % k for k in new) or "none", ", ".join(gone) or "none", ", ".join(changed) or "none"), "",
              "| step kernel | before: VGPR / AGPR / SGPR / spilled VGPR / LDS B / scratch B | after |", "|---|---|---|"]
        for k in sorted(before):
            if "step" in k or "rollout" in k:
                L.append("| %s | %s | %s |" % (k, " / ".join(str(x) for x in before[k]), " / ".join(str(x) for x in now.get(k, ()))))
    return "\n".join(L) + "\n"


def horizon_bench(args):
    """--horizon: DM_OPT_HORIZON_TERMINATION off against on.  A window is one `--steps`-step dm_batch_rollout with the fused policy step (walk, 5-term
    reward, RSI auto-reset, the "deepmimic" fall set) closed by a device synchronise; the option's two values ALTERNATE in one process, `--reps` windows
    each after a warm-up rollout per value.  A third leg, `plain`, is the horizon launch WITHOUT termination on the same workload: on / plain is the
    cost of the termination phase plus the shift in episode lengths.  Prints one JSON line per size; the report is profiles/term_horizon.md's."""
    import torch
    from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
    dev = torch.device("cuda", 0)
    T = args.steps
    lines = []
    for n in args.envs:
        pol = MlpPolicy(device=dev, seed=2); pol.seed(5)
        W = pol.pack()
        ac = torch.zeros((T + 1, n, 28), dtype=torch.float64, device=dev)
        out = (torch.zeros((T, n, 56), dtype=torch.float64, device=dev), torch.zeros((T, n), dtype=torch.float64, device=dev), torch.zeros((T, n), dtype=torch.uint8, device=dev))
        vp = torch.zeros((T, n), dtype=torch.float32, device=dev)
        legs = {"off": dict(fall_contact_bodies="deepmimic", horizon_termination=False), "on": dict(fall_contact_bodies="deepmimic", horizon_termination=True), "plain": {}}
        envs = {k: DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, packed=True, **kw) for k, kw in legs.items()}
        ms = {k: [] for k in legs}
        dones, redo = {}, {}
        for rep in range(args.reps + 1):                                 # (window 0 of every leg is its warm-up)
            for k, env in envs.items():
                b = env.batch
                env.reset("rsi")
                r0 = b.redo_total()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                b.rollout(ac, out, env.frame_skip, W, vp, True, 5, 7)
                b.join(); torch.cuda.synchronize()
                if rep:
                    ms[k].append(1e3 * (time.perf_counter() - t0))
                dones[k] = int(out[2].sum().item()); redo[k] = b.redo_total() - r0
        stats = envs["on"].batch.queue_stats()
        for env in envs.values():
            env.close()
        row = dict(envs=n, steps=T, device=torch.cuda.get_device_name(0))
        for k in legs:
            v = sorted(ms[k])
            row[k] = dict(median_ms=round(float(np.median(v)), 3), min_ms=round(v[0], 3), max_ms=round(v[-1], 3),
                          menv_steps_per_s=round(n * T / float(np.median(v)) / 1e3, 3), episodes_ended=dones[k], restepped_env_steps=redo[k])
        row["on_over_off"] = round(row["off"]["median_ms"] / row["on"]["median_ms"], 3)
        row["on_over_plain_time"] = round(row["on"]["median_ms"] / row["plain"]["median_ms"], 3)
        # the phase reuses a wave's carried kinematics unless one of its environments was re-stepped in that step (5-term reward): at most one wave-step per re-stepped env-step recomputes
        row["wave_steps"] = (n + 3) // 4 * T
        row["wave_steps_recomputed_at_most"] = redo["on"]
        row["queue_stats_on"] = stats
        print(json.dumps(row)); sys.stdout.flush()
        lines.append(row)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", action="store_true", help="DM_OPT_HORIZON_TERMINATION off / on / the horizon launch without termination, alternating (--steps = the horizon, default 128)")
    ap.add_argument("--envs", type=int, nargs="*", default=[4096, 8192])
    ap.add_argument("--steps", type=int, default=None, help="steps per window (default 200; --horizon: the horizon, default 128)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--stats", nargs="*", default=[])
    ap.add_argument("--resources-before", default=None)
    ap.add_argument("--ab", default=None)
    ap.add_argument("--truncation-log", action="store_true", help="measure the truncation log (time limit on, the log off / on) and append the section to --out")
    ap.add_argument("--limit", type=int, default=10, help="--truncation-log: max_episode_steps")
    ap.add_argument("--train-json", default=None, help="--truncation-log: a file of training iteration times to quote")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "term_kernels.md"))
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 128 if args.horizon else 200
    if args.horizon:
        horizon_bench(args)
        return
    if args.trace:
        trace_run(args.trace, args.steps, args.warmup, args)
        return
    import torch
    results = [measure(n, args) for n in args.envs]
    stats = [(int(s.split("=")[0]), s.split("=", 1)[1]) for s in args.stats]
    if args.truncation_log:
        open(args.out, "a").write(report_log(results, stats, args, torch.cuda.get_device_name(0)))
        print(json.dumps(dict(results=results, out=args.out)))
        return
    txt = report(results, stats, args, torch.cuda.get_device_name(0))
    open(args.out, "w").write(txt)
    print(json.dumps(dict(results=results, out=args.out)))


if __name__ == "__main__":
    main()
