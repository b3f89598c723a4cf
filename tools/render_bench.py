#!/usr/bin/env python3
"""Timing of dm_batch_render on one GPU: device-event time per call with device outputs, after a warm-up, for
4 096 views x 128 x 128, 64 views x 256 x 256 and 1 view x 640 x 480 from the side camera (rgb only, and rgb + depth + segmentation),
and the host-visible time of DPEnv.render(mode="rgb_array") at 640 x 480 including the copy to the host.  Poses: frames of the walk
clip spread over the views.  Prints one JSON line.   usage: python tools/render_bench.py [--iters 50] [--warmup 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CASES = [(4096, 128, 128), (64, 256, 256), (1, 640, 480)]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--camera", default="side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from deepmimic_mujoco_amd import Batch, DPEnv
    from deepmimic_mujoco_amd.humanoid import humanoid_spec
    from deepmimic_mujoco_amd.mocap import MocapDM
    from deepmimic_mujoco_amd.model import CompiledModel
    dev = torch.device("cuda", 0)
    mc = MocapDM(); mc.load_mocap("walk")
    cm = CompiledModel(humanoid_spec())
    res = dict(metric="dm_batch_render", camera=args.camera, iters=args.iters, device=torch.cuda.get_device_name(0), cases=[])
    for n, W, H in CASES:
        b = Batch(cm, mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt))
        idx = np.arange(n) % mc.data_config.shape[0]
        b.set_state(mc.data_config[idx], mc.data_vel[idx])
        for extra in (False, True):
            out = dict(rgb=torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev))
            if extra:
                out["depth"] = torch.empty((n, H, W), dtype=torch.float32, device=dev)
                out["segmentation"] = torch.empty((n, H, W), dtype=torch.int32, device=dev)
            for _ in range(args.warmup):
                b.render(W, H, args.camera, depth=extra, segmentation=extra, out=out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                b.render(W, H, args.camera, depth=extra, segmentation=extra, out=out)
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.iters
            rays = n * W * H
            res["cases"].append(dict(views=n, width=W, height=H, outputs="rgb+depth+seg" if extra else "rgb", ms_per_call=round(ms, 4),
                                     rays=rays, grays_per_s=round(rays / (ms * 1e-3) / 1e9, 3)))
        b.close()
    env = DPEnv(motion="walk", device=0)
    for _ in range(args.warmup):
        env.render("rgb_array", 640, 480)
    t = []
    for _ in range(args.iters):
        t0 = time.perf_counter(); img = env.render("rgb_array", 640, 480); t.append(time.perf_counter() - t0)
    assert img.shape == (480, 640, 3)
    res["dpenv_render_640x480_ms"] = dict(median=round(1e3 * float(np.median(t)), 4), min=round(1e3 * float(np.min(t)), 4))
    env.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
