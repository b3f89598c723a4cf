#!/usr/bin/env python3
"""Cost of external pushes on a random schedule (dm_batch_set_push_schedule; csrc/push_kernel.h, kernels_push.hip) on one MI355X, written as
profiles/push_kernels.md.

  throughput   DPVecEnv.step env-steps/s (device tensors, per-step launches on one stream, a window closed by a device synchronise) of a `walk` batch
               with the schedule off and with schedules under which about 0 %, 10 % and 100 % of the environments are pushed at a step, ALTERNATING in one
               process, `--reps` windows each (median and spread), on the one-env and on the packed (DM_OPT_PACKED) per-step kernels: 4 096 envs, reward
               "alive", RSI auto-reset.  The shares come from the schedule itself: a wait of 10^6 steps (the launch runs, every wave returns after its
               bookkeeping), waits of 0..18 steps around one-step pushes (one env in ten at a step once the waits have mixed), no wait at all.
  k_push       the launch's cost per step: the window's time per step against the schedule-off window's, in microseconds.
  resources    registers, spills, scratch and LDS of the two push kernels from the library's code objects (tools/kernel_resources.py; `--resources-only`).

`--bench-lines file`: the default benchmark's JSON result lines of alternating runs of this commit and its parent, one per line, each prefixed with
`parent ` or `this ` (with the schedule off no launch is issued: the headline must not move).  Nothing here is a pass bar.
usage: python tools/push_bench.py [--envs 4096] [--steps 200] [--warmup 40] [--reps 5] [--bench-lines file] [--resources-only] [--out profiles/push_kernels.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources as KR                                        # noqa: E402
from state_bench import buffers                                      # noqa: E402
from terms_bench import bench_section                                # noqa: E402

BODIES = "deepmimic"
SCHEDULES = {"off": None,
             "on, 0 % pushing": dict(bodies=BODIES, force=(50.0, 200.0), duration=(1, 1), wait=(10 ** 6, 10 ** 6)),
             "on, 10 % pushing": dict(bodies=BODIES, force=(50.0, 200.0), duration=(1, 1), wait=(0, 18)),
             "on, 100 % pushing": dict(bodies=BODIES, force=(50.0, 200.0), duration=(1, 1), wait=(0, 0))}


def measure(n, packed, args):
    import torch
    from deepmimic_mujoco_amd import DPVecEnv
    dev = torch.device("cuda", 0)
    envs = {k: DPVecEnv(n, motion="walk", device=0, reward="alive", autoreset="rsi", seed=1, packed=packed, perturb=s) for k, s in SCHEDULES.items()}
    out = buffers(n, 56, dev)
    g = torch.Generator(device=dev); g.manual_seed(5)
    ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * 0.1
    rates = {k: [] for k in envs}
    order = list(envs)
    for rep in range(args.reps):
        for k in order[rep % len(order):] + order[:rep % len(order)]:
            env = envs[k]
            env.reset("rsi")
            for _ in range(args.warmup):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                env.step(ac, out=out)
            torch.cuda.synchronize()
            rates[k].append(n * args.steps / (time.perf_counter() - t0))
    res = {}
    for k, env in envs.items():
        # the share of envs pushed at a step, from the schedule's means: steps held over steps held + steps waited
        p = env.perturb
        share = 0.0 if p is None else 0.5 * sum(p.duration) / (0.5 * sum(p.duration) + 0.5 * sum(p.wait))
        res[k] = dict(median=float(np.median(rates[k])), min=float(min(rates[k])), max=float(max(rates[k])), share=share, packed=bool(env.packed))
        env.close()
    return res


def resources_section(lib):
    rows = {r["name"]: r for r in KR.kernels(lib)}
    L = ["## Resources of the push kernels (`%s`, tools/kernel_resources.py)" % os.path.relpath(lib, ROOT), "",
         "| kernel | VGPRs (of which AGPRs) | spilled VGPRs | spilled SGPRs | scratch bytes per lane | LDS bytes |", "|---|---|---|---|---|---|"]
    for name in ("k_push", "k_push_now"):
        r = rows.get(name)
        L.append("| %s | %s |" % (name, "—" if r is None else "%d (%d) | %d | %d | %d | %d" % (r["vgpr"], r["agpr"], r["vspill"], r["sspill"], r["scratch"], r["lds"])))
    return L + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "libdmenv.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "push_kernels.md"))
    args = ap.parse_args()
    L = ["# External pushes: what the schedule's launch costs (`tools/push_bench.py`)", ""]
    if not args.resources_only:
        for packed, title in ((False, "one env per wave"), (True, "DM_OPT_PACKED, four envs per wave")):
            res = measure(args.envs, packed, args)
            off = res["off"]["median"]
            L += ["## Throughput: DPVecEnv.step, %d `walk` envs, %s, reward \"alive\", RSI auto-reset, frame_skip 1" % (args.envs, title), "",
                  "%d windows of %d steps each after %d warm-up steps, the four batches alternating in one process; env-steps/s.  k_push per step: the window's time per"
                  " step minus the schedule-off window's (medians)." % (args.reps, args.steps, args.warmup), "",
                  "| schedule | envs pushed at a step (the schedule's mean) | median | min | max | against off | k_push per step |", "|---|---|---|---|---|---|---|"]
            for k, r in res.items():
                L.append("| %s | %.2g | %.3f M | %.3f M | %.3f M | %.3f | %s |" % (k, r["share"], r["median"] / 1e6, r["min"] / 1e6, r["max"] / 1e6, r["median"] / off,
                                                                               "—" if k == "off" else "%.1f us" % ((args.envs / r["median"] - args.envs / off) * 1e6)))
            L.append("")
        L += ["A pushed environment also steps differently afterwards (other contacts, other constraint rows), so the 10 % and 100 % rows hold the launch and what the pushes"
              " do to the population; the 0 % row is the launch alone.  Reported, not gated.", ""]
        L += [x.replace(" with the option off", " with the schedule off") for x in bench_section(args.bench_lines)]
    L += resources_section(args.lib)
    txt = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
