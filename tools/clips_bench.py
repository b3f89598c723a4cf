#!/usr/bin/env python3
"""Cost of a multi-clip batch (dm_mocap_create_set: one clip per env; csrc/kernels_clips.hip, kernels_packed_clips.hip) on one MI355X, written as
profiles/clips_kernels.md.

  throughput   DPVecEnv.step env-steps/s (device tensors, per-step launches on one stream, a window closed by a device synchronise) of a
               single-clip batch (`walk`), a 3-clip batch (walk, spinkick, kick) and a 15-clip batch (every bundled clip), ALTERNATING in one process,
               `--reps` windows each (median and spread): 4 096 envs, the 5-term imitation reward (reward mode 3), DM_OPT_PACKED, RSI auto-reset,
               clip mode "episode" on the clip sets.  The ratio is reported, not gated.
  resources    registers, spills, scratch and LDS of the clip kernels beside their single-clip twins, from the library's code objects
               (tools/kernel_resources.py; no GPU needed: `--resources-only`).

`--bench-lines file`: the default benchmark's JSON result lines of alternating runs of this commit and its parent, one per line, each prefixed
with `parent ` or `this `.  `--resources-before file.md`: the table tools/kernel_resources.py printed for the parent's library.
usage: python tools/clips_bench.py [--envs 4096] [--steps 200] [--warmup 30] [--reps 5] [--bench-lines file] [--resources-before file.md]
                                   [--resources-only] [--out profiles/clips_kernels.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources as KR                                        # noqa: E402
from state_bench import buffers, parse_before                        # noqa: E402
from terms_bench import bench_section                                # noqa: E402

SETS = {"1 clip": "walk", "3 clips": ["walk", "spinkick", "kick"], "15 clips": None}      # None: every bundled clip
TWINS = [("k_step_packed_clips", "k_step_packed", "k_step_packed_spd"), ("k_step_packed_ext_clips", "k_step_packed_ext", "k_step_packed_ext_spd"),
         ("k_step_packed_act_clips", "k_step_packed_act", "k_step_packed_act_spd"), ("k_step_packed_act_ext_clips", "k_step_packed_act_ext", "k_step_packed_act_ext_spd"),
         ("k_step_narrow_clips", "k_step_narrow", "k_step_narrow_spd"), ("k_step_act_clips", "k_step_act", "k_step_act_spd"), ("k_step_clips", "k_step", "k_step_spd"),
         ("k_step_redo_clips", "k_step_redo", "k_step_redo_spd"), ("k_reset_clips", "k_reset", None), ("k_terminate_clips", "k_terminate", None),
         ("k_state_features_clips", "k_state_features", None), ("k_imitation_terms_clips", "k_imitation_terms", None)]


def make_env(n, motion):
    from deepmimic_mujoco_amd import DPVecEnv
    from deepmimic_mujoco_amd.mocap import ALL_CLIPS
    if motion is None:
        motion = list(ALL_CLIPS)
    many = isinstance(motion, list)
    return DPVecEnv(n, motion=motion, device=0, reward="imitation", autoreset="rsi", seed=1, packed=True, clip_mode="episode" if many else "fixed")


def measure(n, args):
    import torch
    dev = torch.device("cuda", 0)
    envs = {k: make_env(n, m) for k, m in SETS.items()}
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
        res[k] = dict(median=float(np.median(rates[k])), min=float(min(rates[k])), max=float(max(rates[k])), frame_skip=env.frame_skip, packed=bool(env.packed))
        env.close()
    return res


def resources_section(lib, before):
    rows = {r["name"]: r for r in KR.kernels(lib)}
    cell = lambda r: "—" if r is None else "%d (%d) / %d / %d / %d / %d" % (r["vgpr"], r["agpr"], r["vspill"], r["sspill"], r["scratch"], r["lds"])
    L = ["## Resources of the clip kernels beside their single-clip twins (`%s`, tools/kernel_resources.py)" % os.path.relpath(lib, ROOT), "",
         "Each cell: VGPRs, unified total (of which AGPRs) / spilled VGPRs / spilled SGPRs / scratch bytes per lane / LDS bytes.  A clip step kernel holds BOTH"
         " controller instantiations (it picks stable PD by the batch's action mode at run time), so its twin is the larger of the two single-clip kernels.", "",
         "| clip kernel | its resources | twin, action modes 0..2 | twin, action modes 3 and 4 |", "|---|---|---|---|"]
    for name, twin, spd in TWINS:
        L.append("| %s | %s | %s: %s | %s |" % (name, cell(rows.get(name)), twin, cell(rows.get(twin)), "—" if spd is None else "%s: %s" % (spd, cell(rows.get(spd)))))
    L.append("")
    if before and os.path.exists(before):
        old = parse_before(open(before).read())
        changed = [k for k, v in old.items() if k not in rows or v != (rows[k]["vgpr"], rows[k]["agpr"], rows[k]["sgpr"], rows[k]["vspill"], rows[k]["lds"], rows[k]["scratch"])]
        L += ["Pre-existing kernels against the parent's library (%d kernels): %s." % (len(old), "all identical" if not changed else "CHANGED: " + ", ".join(changed)), ""]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bench-lines", default=None)
    ap.add_argument("--resources-before", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "deepmimic_mujoco_amd", "csrc", "libdmenv.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_kernels.md"))
    args = ap.parse_args()
    L = ["# Multi-clip batches: what one clip per env costs (`tools/clips_bench.py`)", ""]
    if not args.resources_only:
        res = measure(args.envs, args)
        base = res["1 clip"]["median"]
        L += ["## Throughput: DPVecEnv.step, %d envs, imitation reward, DM_OPT_PACKED per-step launches, RSI auto-reset, frame_skip %d" % (args.envs, res["1 clip"]["frame_skip"]), "",
              "%d windows of %d steps each after %d warm-up steps, the three batches alternating in one process; env-steps/s." % (args.reps, args.steps, args.warmup), "",
              "| batch | median | min | max | against the single-clip batch |", "|---|---|---|---|---|"]
        for k, r in res.items():
            L.append("| %s | %.3f M | %.3f M | %.3f M | %.3f |" % (k, r["median"] / 1e6, r["min"] / 1e6, r["max"] / 1e6, r["median"] / base))
        L += ["", "The clips differ in content as well as in kernel: another motion holds other contacts, and the step's cost follows its constraint rows.  The figure is"
              " what a user of a clip set sees; it is reported, not gated.", ""]
        # (terms_bench's section speaks of its option; here: a single-clip batch, which launches none of the clip kernels)
        L += [x.replace(" with the option off", "").replace("nothing is launched or allocated", "a single-clip batch launches none of the new kernels") for x in bench_section(args.bench_lines)]
    L += resources_section(args.lib, args.resources_before)
    txt = "\n".join(L) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(txt)
    print(txt)


if __name__ == "__main__":
    main()
