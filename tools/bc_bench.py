#!/usr/bin/env python3
"""Behaviour-cloning iteration timing (profiles/bc_kernels.md): microseconds per BC iteration at the given batch sizes for three paths —
  fused     dm_bc_fit: `--iters` iterations enqueued by one call (k_pg<BC> + k_bc_adam per iteration, nothing back to the host)
  periter   dm_bc_lossgrad + MpiAdam per iteration (behavior_clone.learn's multi-rank path, on one process)
  autograd  torch autograd + MpiAdam per iteration on the GPU (behavior_clone.learn with native=False)
Wall time on a host clock around synchronised runs of `--iters` iterations after `--warmup` iterations of the same path.  The batches are
pre-drawn indices into a synthetic expert set, so the host's Dset bookkeeping is not timed.  Per-kernel times: run under
rocprofv3 --kernel-trace --stats.
Usage: python tools/bc_bench.py [--bs 128 1024] [--iters 10000] [--warmup 200] [--paths fused periter autograd] [--out x.json]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from deepmimic_mujoco_amd import MlpPolicy  # noqa: E402
from deepmimic_mujoco_amd import behavior_clone as BC  # noqa: E402
from deepmimic_mujoco_amd.trpo import POL_KEYS, MpiAdam  # noqa: E402

DEV = torch.device("cuda", 0)


class _Expert:
    def __init__(self, n, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.obs = torch.randn(n, 56, generator=g).to(DEV)
        self.acs = torch.tanh(torch.randn(n, 28, generator=g) * 0.5).to(DEV)


def run(path, bs, iters, warmup, expert, rows):
    pi = MlpPolicy(device=DEV, seed=0)
    pol = [pi.params[k] for k in POL_KEYS]
    K = BC._Kernels(pi, expert, bs, 1)
    rng = np.random.RandomState(bs)
    idx = torch.from_numpy(rng.randint(0, rows, size=(warmup + iters, bs)).astype(np.int32)).to(DEV)
    idx64 = idx.to(torch.int64)
    adam = MpiAdam(pol, epsilon=1e-5)
    if path == "fused":
        theta = adam.getflat().contiguous()

        def go(a, b):
            scales = [3e-4 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) for t in range(a + 1, b + 1)]
            K.fit(theta, adam.m, adam.v, idx[a:b], scales, 0.9, 0.999, 1e-5, a)
    elif path == "periter":
        def go(a, b):
            for it in range(a, b):
                _, g = K.lossgrad(adam.getflat().contiguous(), idx[it], it)
                adam.update(g, 3e-4)
    else:
        def go(a, b):
            for it in range(a, b):
                r = idx64[it]
                _, g = BC._torch_lossgrad(pi, expert.obs.index_select(0, r), expert.acs.index_select(0, r), 1, it)
                adam.update(g, 3e-4)
    go(0, warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go(warmup, warmup + iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 1024])
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--paths", nargs="+", default=["fused", "periter", "autograd"], choices=["fused", "periter", "autograd"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    rows = 50000
    expert = _Expert(rows)
    res = []
    for bs in args.bs:
        for path in args.paths:
            us = run(path, bs, args.iters, args.warmup, expert, rows)
            res.append(dict(path=path, bs=bs, iters=args.iters, us_per_iter=us))
            print("bs %5d  %-8s  %8.1f us per iteration  (%d iterations: %.3f s)" % (bs, path, us, args.iters, us * args.iters * 1e-6), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(dict(device=torch.cuda.get_device_name(DEV), results=res), open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
