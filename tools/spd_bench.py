#!/usr/bin/env python3
"""Cost of the PD-target action modes (DM_OPT_ACTION_MODE 3 "spd-target", 4 "spd-mocap": a stable PD controller evaluated at every simulation
substep inside the step kernels) next to the modes that existed before, on one GPU: closed-loop DPVecEnv.step env-steps/s — every step's outputs
joined before the next call — at 4 096 `walk` envs with full contacts + limits, the 5-term imitation reward and RSI auto-reset, for
n_substeps 1 and 2, action modes raw / pd / spd-target / spd-mocap, one env per wave and four per wave (DM_OPT_PACKED).  Actions: N(0, sigma^2)
noise — a motor command (raw), an offset from the mocap frame (pd, spd-mocap) or an offset from the clip's first pose (spd-target).  Each case is
timed `--reps` times (median and spread reported); the figure to hold the new modes against is `pd` of the same call.  Prints one JSON line.
usage: python tools/spd_bench.py [--envs 4096] [--steps 200] [--warmup 30] [--reps 3] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MODES = ["raw", "pd", "spd-target", "spd-mocap"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from deepmimic_mujoco_amd import DPVecEnv
    dev = torch.device("cuda", 0)
    n = args.envs
    res = dict(metric="DPVecEnv.step env-steps/s, closed loop", envs=n, steps=args.steps, reps=args.reps, sigma=args.sigma, clip="walk", reward="imitation",
               device=torch.cuda.get_device_name(0), cases=[])
    for packed in (False, True):
        for nsub in (1, 2):
            row = {}
            for mode in MODES:
                env = DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, frame_skip=nsub, action_mode=mode, packed=packed)
                b = env.batch
                g = torch.Generator(device=dev); g.manual_seed(5)
                ac = torch.randn((n, 28), generator=g, dtype=torch.float64, device=dev) * args.sigma
                if mode == "spd-target":
                    ac += torch.as_tensor(env.mocap.data_config[0][7:], device=dev)
                out = (torch.zeros((n, 56), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
                rates, redo0 = [], b.redo_total()
                for rep in range(args.reps):
                    env.reset("rsi")
                    for _ in range(args.warmup):
                        b.step(ac, nsub, out); b.join()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.steps):
                        b.step(ac, nsub, out); b.join()
                    torch.cuda.synchronize()
                    rates.append(n * args.steps / (time.perf_counter() - t0))
                assert bool(torch.isfinite(out[0]).all())
                row[mode] = float(np.median(rates))
                res["cases"].append(dict(packed=packed, n_substeps=nsub, action_mode=mode, env_steps_per_s=round(float(np.median(rates))),
                                         min=round(min(rates)), max=round(max(rates)), redo_per_env_step=round((b.redo_total() - redo0) / float(n * args.reps * (args.steps + args.warmup)), 5)))
                env.close()
            for mode in ("spd-target", "spd-mocap"):
                res["cases"].append(dict(packed=packed, n_substeps=nsub, ratio="%s / pd" % mode, value=round(row[mode] / row["pd"], 4)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
