"""Behaviour cloning of the policy on the expert's transitions: the `behavior_clone.learn(env, policy_fn, dataset, max_iters=BC_max_iter)` that
src/gail.py:490-495 calls for `--pretrained` before GAIL starts from the cloned weights (:131, :227-229).  The reference imports the module but
does not ship it; its semantics are those of OpenAI baselines' GAIL, where that gail.py comes from:

    loss  = mean over batch x 28 of (ac_expert - pi.ac)^2,  pi.ac = mean + exp(logstd) eps (the STOCHASTIC action, so logstd is trained too)
    adam  = MpiAdam(pi.get_trainable_variables(), epsilon=1e-5), stepsize 3e-4, batch 128, `max_iters` iterations
    one iteration: ob, ac = dataset.get_next_batch(128, 'train'); loss, g = lossandgrad(ob, ac, True); adam.update(g, 3e-4)
    verbose: every int(max_iters / 10) iterations also the loss on the whole val split (get_next_batch(-1, 'val'))

The value net's gradient is zero, so its Adam moments and steps stay zero: only the policy's flat parameters (TrpoLearner.get_flat order,
dm_pg_param_count() floats) are optimised here, and the value parameters come out bit-identical.  The obs filter is not updated (the reference
does not: a fresh policy normalises with mean 0, std 1, clipped to +-5).  eps is the device's counter noise normal_from(seed, counter, s * 28 + a)
(csrc/rng.h) with its own seed; the torch path takes it from the host mirror `normal_from` below.

Paths:  one process on a GPU: dm_bc_fit, `chunk` iterations per call (two launches per iteration, nothing comes back to the host);
        several processes: dm_bc_lossgrad + MpiAdam per iteration (the gradient is all-mean'd across ranks);
        CPU tensors or native=False: torch autograd + MpiAdam.
The expert's shuffles (`expert.rng`) are restored after BC, so GAIL draws the same expert batches with and without pretraining.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _abi as A
from .trpo import POL_KEYS, MpiAdam, _world, native_nets

AC = 28
_M64 = (1 << 64) - 1
NOISE_SEED_XOR = 0xB0C10E5EED            # BC's noise stream is apart from the rollout's act() noise of the same seed
VAL_COUNTER = 1 << 40                    # the val loss after iteration i draws counter VAL_COUNTER + i


def _mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def normal_from(seed, counter, idx):
    """Host mirror of csrc/rng.h normal_from for an array of element indices: float64 Box-Muller on the same 24-bit uniforms."""
    with np.errstate(over="ignore"):
        base = _mix64(np.uint64(int(seed) & _M64) ^ np.uint64((int(counter) * 0xD1342543DE82EF95) & _M64))
        h = _mix64(base + np.asarray(idx, dtype=np.uint64))
    u1 = ((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float64) + 1.0
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64)
    return np.sqrt(-2.0 * np.log(u1 / 16777216.0)) * np.cos(2.0 * math.pi * (u2 / 16777216.0))


def _native_ok(pi, native):
    if native is False or pi.device.type != "cuda":
        return False
    ok = native_nets(pi, POL_KEYS)
    if not ok and native is True:
        raise ValueError("the BC kernels need the 56-100-100-28 float32 policy on a GPU")
    return ok


class _Kernels:
    """dm_bc_lossgrad / dm_bc_fit on the policy's device."""

    def __init__(self, pi, expert, bs, noise_seed):
        self.L = A.load()
        self.pi, self.dev, self.seed = pi, pi.device, noise_seed
        assert self.L.dm_pg_param_count() == sum(pi.params[k].numel() for k in POL_KEYS)
        self.ob = expert.obs.to(self.dev, torch.float32).contiguous()
        self.ac = expert.acs.to(self.dev, torch.float32).contiguous()
        self.scratch = None
        self.reserve(bs)

    def reserve(self, n):
        self.scratch = A.scratch(self.scratch, self.L.dm_bc_scratch_bytes(int(n)), self.dev)

    def lossgrad(self, theta, idx_dev, counter, grad=True):
        """-> (loss [1] float64, flat gradient or None) on the device; idx_dev: int32 device rows."""
        n = int(idx_dev.numel())
        self.reserve(n)
        rms = self.pi.ob_rms
        loss = torch.empty(1, dtype=torch.float64, device=self.dev)
        g = torch.empty(theta.numel(), dtype=torch.float32, device=self.dev) if grad else None
        p = A.ptr
        A.check(self.L.dm_bc_lossgrad(p(self.ob), p(self.ac), p(idx_dev), n, p(theta), p(rms.mean), p(rms.std), 1, self.seed & _M64, int(counter) & _M64,
                                      p(g), p(loss), p(self.scratch), self.scratch.numel(), A.stream(self.dev)), self.L)
        return loss, g

    def fit(self, theta, m, v, idx_dev, scales, beta1, beta2, eps, counter0):
        """len(scales) iterations of dm_bc_fit on idx_dev [iters, bs]; -> losses [iters] float64 on the device."""
        iters, bs = int(idx_dev.shape[0]), int(idx_dev.shape[1])
        self.reserve(bs)
        rms = self.pi.ob_rms
        out = torch.empty(iters, dtype=torch.float64, device=self.dev)
        sc = (C.c_float * iters)(*scales)
        p = A.ptr
        A.check(self.L.dm_bc_fit(p(self.ob), p(self.ac), p(idx_dev), iters, bs, p(theta), p(m), p(v), sc, float(beta1), float(beta2), float(eps),
                                 p(rms.mean), p(rms.std), 1, self.seed & _M64, int(counter0) & _M64, p(out), p(self.scratch), self.scratch.numel(),
                                 A.stream(self.dev)), self.L)
        return out


def _torch_lossgrad(pi, ob, ac, seed, counter, grad=True, stochastic=True):
    """The loss of one batch by torch autograd (float32), eps from the host mirror of the device noise (zero: stochastic=False)."""
    n = ob.shape[0]
    eps = normal_from(seed, counter, np.arange(n * AC, dtype=np.uint64)).reshape(n, AC) if stochastic else np.zeros((n, AC))
    eps = torch.as_tensor(eps, dtype=torch.float32, device=pi.device)
    pol = [pi.params[k].detach().clone().requires_grad_(grad) for k in POL_KEYS]
    saved = {k: pi.params[k] for k in POL_KEYS}
    try:
        for k, t in zip(POL_KEYS, pol):
            pi.params[k] = t
        with torch.enable_grad() if grad else torch.no_grad():
            acs = pi.forward_mean(ob) + torch.exp(pol[-1]) * eps
            loss = ((ac.to(torch.float32) - acs) ** 2).mean()
            g = torch.cat([x.reshape(-1) for x in torch.autograd.grad(loss, pol)]) if grad else None
    finally:
        pi.params.update(saved)
    return loss.detach().to(torch.float64).reshape(1), g


def learn(pi, expert, *, max_iters=10000, optim_batch_size=128, optim_stepsize=3e-4, adam_epsilon=1e-5, verbose=False, seed=0, group=None,
          native=None, chunk=1000, log=print):
    """Train `pi` (an MlpPolicy) in place on `expert` (gail.ExpertDataset) for `max_iters` iterations of `optim_batch_size` rows.
    Returns (train_losses: float64 array [max_iters], each iteration's loss before its step; val: list of (iteration, val loss) pairs, with
    `verbose` only).  A train split smaller than the batch gives batches of that smaller, constant size (Dset semantics).
    native: None = the kernels when they can run, False = torch, True = the kernels or an error.  chunk: iterations per dm_bc_fit call."""
    max_iters, bs = int(max_iters), int(optim_batch_size)
    if max_iters < 1 or bs < 1:
        raise ValueError("max_iters and optim_batch_size must be >= 1")
    if expert.train_set.num_pairs < 1:
        raise ValueError("the expert's train split is empty")
    val_per_iter = max(1, int(max_iters / 10))
    noise_seed = (int(seed) ^ NOISE_SEED_XOR) & _M64
    world = _world(group)
    use_kernels = _native_ok(pi, native)
    pol = [pi.params[k] for k in POL_KEYS]
    rng_state = expert.rng.get_state()
    val_idx = np.asarray(expert.next_indices(-1, "val"))
    train, val = [], []

    def report(it, loss, vloss):
        val.append((it, vloss))
        if log:
            log("BC iter %6d  train loss %.6f  val loss %.6f" % (it, loss, vloss))

    if use_kernels and world == 1:
        K = _Kernels(pi, expert, bs, noise_seed)
        adam = MpiAdam(pol, epsilon=adam_epsilon)
        theta = adam.getflat().to(torch.float32).contiguous()
        vidx = torch.from_numpy(val_idx.astype(np.int32)).to(pi.device) if verbose and len(val_idx) else None
        it = 0
        while it < max_iters:
            end = min(max_iters, it + int(chunk))
            if verbose:                                                 # a chunk ends with each iteration that reports the val loss
                end = min(end, -(-it // val_per_iter) * val_per_iter + 1)
            idx = np.stack([np.asarray(expert.next_indices(bs, "train")) for _ in range(it, end)]).astype(np.int32)
            train.append(K.fit(theta, adam.m, adam.v, torch.from_numpy(idx).to(pi.device), adam.stepsizes(optim_stepsize, end - it), adam.beta1, adam.beta2, adam_epsilon, it))
            adam.t += end - it
            it = end
            if verbose and (it - 1) % val_per_iter == 0 and vidx is not None:
                vloss, _ = K.lossgrad(theta, vidx, VAL_COUNTER + it - 1, grad=False)
                report(it - 1, float(train[-1][-1]), float(vloss))
        adam.setfromflat(theta)
        train = torch.cat(train).cpu().numpy()
    else:
        K = _Kernels(pi, expert, bs, noise_seed) if use_kernels else None
        adam = MpiAdam(pol, epsilon=adam_epsilon, group=group)
        adam.sync()
        ob_all, ac_all = expert.obs.to(pi.device), expert.acs.to(pi.device)

        def lossgrad(rows, counter, grad=True):
            if K is not None:
                return K.lossgrad(adam.getflat().to(torch.float32).contiguous(), torch.from_numpy(np.asarray(rows, dtype=np.int32)).to(pi.device),
                                  counter, grad)
            r = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(pi.device)
            return _torch_lossgrad(pi, ob_all.index_select(0, r), ac_all.index_select(0, r), noise_seed, counter, grad)

        for it in range(max_iters):
            loss, g = lossgrad(expert.next_indices(bs, "train"), it)
            adam.update(g, optim_stepsize)
            train.append(loss)
            if verbose and it % val_per_iter == 0 and len(val_idx):
                vloss, _ = lossgrad(val_idx, VAL_COUNTER + it, grad=False)
                report(it, float(loss), float(vloss))
        train = torch.cat(train).cpu().numpy()
    expert.rng.set_state(rng_state)
    pi.mark_dirty()
    return train, val
