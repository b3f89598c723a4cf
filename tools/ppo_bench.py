#!/usr/bin/env python3
"""PPO timing (profiles/ppo_kernels.md), three paths of deepmimic_mujoco_amd.ppo on one GPU:
  fused     dm_ppo_fit: a chunk of minibatches enqueued by one call (k_pg<PPO> + k_vf_grad_rows + k_ppo_step per minibatch, nothing back to the host)
  periter   dm_ppo_lossgrad + MpiAdam per minibatch (the multi-rank path, on one process)
  autograd  torch autograd + MpiAdam per minibatch on the GPU (native=False)
(1) microseconds per minibatch at the given batch sizes: wall time on a host clock around a synchronised run of `--iters` minibatches
    (autograd: a tenth of them) after `--warmup`, rows pre-drawn from a synthetic segment of `--rows` rows;
(2) one whole update (PpoLearner.update_batch: obs filter, old policy, `--epochs` epochs of minibatches of `--update-bs`, the loss pass) on a
    segment of --envs x --horizon rows, one warm-up update first.
Usage: python tools/ppo_bench.py [--bs 64 256 4096] [--iters 2000] [--envs 1024 --horizon 64] [--out x.json]"""
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
from deepmimic_mujoco_amd import ppo  # noqa: E402

DEV = torch.device("cuda", 0)
PATHS = ("fused", "periter", "autograd")


def segment(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    ob = torch.randn(n, 56, generator=g)
    ac = torch.randn(n, 28, generator=g) * 0.5
    adv, ret, vpred = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    return [t.to(DEV).contiguous() for t in (ob, ac, adv, ret, vpred)]


def learner(path, **kw):
    pi = MlpPolicy(device=DEV, seed=0)
    return ppo.PpoLearner(pi, schedule="constant", native=(path != "autograd"), per_minibatch=(path == "periter"), **kw)


def per_minibatch(path, bs, iters, warmup, seg):
    L = learner(path)
    ob, ac, adv, ret, _ = seg
    n = ob.shape[0]
    atarg = ((adv - adv.mean()) / adv.std(unbiased=False)).contiguous()
    with torch.no_grad():
        old_mean = L.pi.forward_mean(ob).contiguous()
    D = dict(ob=ob, ac=ac, atarg=atarg, old_mean=old_mean, old_logstd=L.pi.params["logstd"].detach().reshape(-1).clone(), ret=ret)
    rng = np.random.RandomState(bs)
    idx = torch.from_numpy(rng.randint(0, n, size=(warmup + iters, bs)).astype(np.int32)).to(DEV)
    idx64 = idx.to(torch.int64)
    ad = L.adam
    if path == "fused":
        theta = ad.getflat().contiguous()

        def go(a, b):
            scales = [3e-4 * math.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) for t in range(a + 1, b + 1)]
            L.kernel_fit(D, idx[a:b].contiguous(), bs, theta, ad.m, ad.v, scales, [0.2] * (b - a))
    elif path == "periter":
        def go(a, b):
            for it in range(a, b):
                _, g = L.kernel_lossgrad(D, idx[it], ad.getflat().contiguous(), 0.2)
                ad.update(g, 3e-4)
    else:
        def go(a, b):
            for it in range(a, b):
                _, g = L.torch_lossgrad(D, idx64[it], 0.2)
                ad.update(g, 3e-4)
    go(0, warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    go(warmup, warmup + iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def whole_update(path, seg, bs, epochs):
    L = learner(path, optim_batchsize=bs, optim_epochs=epochs)
    times = []
    for _ in range(2):                                                 # a warm-up update, then the timed one
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stats = L.update_batch(*seg)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times[-1] * 1e3, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[64, 256, 4096])
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--update-bs", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--paths", nargs="+", default=list(PATHS), choices=PATHS)
    ap.add_argument("--no-update", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(DEV)
    seg = segment(args.rows)
    res = dict(device=torch.cuda.get_device_name(DEV), minibatch=[], update=[])
    for bs in args.bs:
        for path in args.paths:
            iters = args.iters if path != "autograd" else max(1, args.iters // 10)
            us = per_minibatch(path, bs, iters, min(args.warmup, iters), seg)
            res["minibatch"].append(dict(path=path, bs=bs, iters=iters, us_per_minibatch=us))
            print("bs %5d  %-8s  %9.1f us per minibatch  (%d minibatches)" % (bs, path, us, iters), flush=True)
    if not args.no_update:
        useg = segment(args.envs * args.horizon, seed=1)
        for path in args.paths:
            ms, stats = whole_update(path, useg, args.update_bs, args.epochs)
            res["update"].append(dict(path=path, rows=args.envs * args.horizon, bs=args.update_bs, epochs=args.epochs, ms=ms,
                                      minibatches=stats["optim_steps"], loss_kl=stats["loss_kl"], clipfrac=stats["clipfrac"]))
            print("update %d x %d rows, bs %d, %d epochs  %-8s  %9.1f ms  (%d minibatches, %.1f us each; loss_kl %.5f)"
                  % (args.envs, args.horizon, args.update_bs, args.epochs, path, ms, stats["optim_steps"], ms * 1e3 / max(1, stats["optim_steps"]),
                     stats["loss_kl"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
