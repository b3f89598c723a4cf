#!/usr/bin/env python3
"""Cost of the PD-target action modes (DM_OPT_ACTION_MODE 3 "spd-target", 4 "spd-mocap": a stable PD controller evaluated at every simulation
substep inside the step kernels) next to the modes that existed before, on one GPU: closed-loop DPVecEnv.step env-steps/s — every step's outputs
joined before the next call — at 4 096 `walk` envs with full contacts + limits, the 5-term imitation reward and RSI auto-reset, for
n_substeps 1 and 2, action modes raw / pd / spd-target / spd-mocap, one env per wave and four per wave (DM_OPT_PACKED).  Actions: N(0, sigma^2)
noise — a motor command (raw), an offset from the mocap frame (pd, spd-mocap) or an offset from the clip's first pose (spd-target).  Each case is
timed `--reps` times (median and spread reported); the figure to hold the new modes against is `pd` of the same call.  Prints one JSON line.
`--horizon`: DM_OPT_HORIZON_SPD (the controller inside the horizon launch) off against on — see horizon_bench; the report is profiles/spd_horizon.md's.
usage: python tools/spd_bench.py [--envs 4096] [--steps 200] [--warmup 30] [--reps 3] [--out file.json]
       python tools/spd_bench.py --horizon [--envs 4096 8192] [--steps 128] [--reps 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

MODES = ["raw", "pd", "spd-target", "spd-mocap"]


def horizon_bench(args):
    """--horizon: DM_OPT_HORIZON_SPD off against on in action mode 3 ("spd-target").  A window is one `--steps`-step dm_batch_rollout with the fused policy step
    (walk, 5-term reward, frame_skip="mocap", RSI auto-reset, DM_OPT_PACKED 1) closed by a device synchronise; the option's two values ALTERNATE in one
    process, `--reps` windows each after a warm-up rollout per value.  Off is one step launch per step with the policy fused into it; on is one launch.
    Then the same with early termination: the "deepmimic" fall set and a 600-step limit — off: step, termination and policy launches per step; on:
    DM_OPT_HORIZON_TERMINATION alongside, one launch.  Prints one JSON line per size and leg."""
    import torch
    from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
    dev = torch.device("cuda", 0)
    T = args.steps
    lines = []
    for n in args.envs:
        pol = MlpPolicy(device=dev, seed=2); pol.seed(5)
        W = pol.pack()
        out = (torch.zeros((T, n, 56), dtype=torch.float64, device=dev), torch.zeros((T, n), dtype=torch.float64, device=dev), torch.zeros((T, n), dtype=torch.uint8, device=dev))
        vp = torch.zeros((T, n), dtype=torch.float32, device=dev)
        for leg, term in (("plain", {}), ("termination", dict(fall_contact_bodies="deepmimic", max_episode_steps=600))):
            envs = {k: DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, packed=True, frame_skip="mocap", action_mode="spd-target",
                                horizon_spd=k == "on", horizon_termination=bool(term) and k == "on", **term) for k in ("off", "on")}
            ac = torch.zeros((T + 1, n, 28), dtype=torch.float64, device=dev)
            ac[0] = torch.as_tensor(envs["on"].mocap.data_config[0][7:], device=dev)      # the first target pose: the clip's; the policy writes the rest
            ms = {k: [] for k in envs}
            dones, redo = {}, {}
            for rep in range(args.reps + 1):                                 # (window 0 of either value is its warm-up)
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
            assert bool(torch.isfinite(out[0]).all())
            nsub = envs["on"].frame_skip
            for env in envs.values():
                env.close()
            row = dict(leg=leg, envs=n, steps=T, n_substeps=nsub, action_mode="spd-target", device=torch.cuda.get_device_name(0))
            for k in ms:
                v = sorted(ms[k])
                row[k] = dict(median_ms=round(float(np.median(v)), 3), min_ms=round(v[0], 3), max_ms=round(v[-1], 3),
                              menv_steps_per_s=round(n * T / float(np.median(v)) / 1e3, 3), episodes_ended=dones[k], restepped_env_steps=redo[k])
            row["on_over_off"] = round(row["off"]["median_ms"] / row["on"]["median_ms"], 3)
            print(json.dumps(row)); sys.stdout.flush()
            lines.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("".join(json.dumps(r) + "\n" for r in lines))
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", action="store_true", help="DM_OPT_HORIZON_SPD off / on, alternating, without and with early termination (--steps = the horizon, default 128; --envs takes several sizes)")
    ap.add_argument("--envs", type=int, nargs="*", default=None)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.steps is None:
        args.steps = 128 if args.horizon else 200
    if args.horizon:
        args.envs = args.envs or [4096, 8192]
        horizon_bench(args)
        return
    args.envs = (args.envs or [4096])[0]
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
