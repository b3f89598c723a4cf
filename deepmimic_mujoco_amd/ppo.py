"""PPO with the clipped surrogate: OpenAI baselines' ppo1 `pposgd_simple.learn`, the learner the reference's policy file comes from
(src/mlp_policy_trpo.py:2) and that its `--algo {trpo,ppo}` flag (src/gail.py:394) names but never runs.  One update on a segment:

    add_vtarg_and_adv(seg, gamma, lam);  atarg = (atarg - mean) / std   [ddof 0, per rank]
    pi.ob_rms.update(ob)                 [once, before any step: the filter stays fixed for the whole update]
    assign_old_eq_new                    [old_mean [n, 28] of every row, old logstd]
    lrmult = 1 (schedule "constant") or max(1 - timesteps_so_far / max_timesteps, 0) ("linear"); clip = clip_param lrmult
    optim_epochs times: a fresh permutation, floor(n / bs) minibatches of bs rows (the tail is dropped: Dataset.iterate_once), each one
        g = grad of pol_surr + pol_entpen + vf_loss w.r.t. the policy AND the value net, MpiAdam(epsilon = adam_epsilon).update(g, optim_stepsize lrmult)
    losses: one more shuffled pass over full minibatches, no step: the mean of [pol_surr, pol_entpen, vf_loss, kl, ent] (+ clipfrac)

    ratio = exp(logp_new(ac) - logp_old(ac)),  pol_surr = -mean(min(ratio A, clip(ratio, 1 - clip, 1 + clip) A)),
    pol_entpen = -entcoeff mean(entropy),  vf_loss = mean((vpred - tdlamret)^2),  kl = mean KL(old || new)  (DiagGaussianPd, src/distributions.py)

min() sends its gradient to its first argument on a tie (TF's `minimum`).  All minibatches have bs rows, so the mean over the loss pass's
minibatches is the mean over its nb * bs rows: the pass is one call.

Paths:  one process on a GPU: dm_ppo_fit, one call per epoch (three launches per minibatch: csrc/pg_kernel.h k_pg<MODE_PPO>, csrc/vf_kernel.h
        k_vf_grad_rows, k_ppo_step; nothing comes back to the host);
        several processes (or per_minibatch=True): dm_ppo_lossgrad + trpo.MpiAdam per minibatch (the gradient is all-mean'd across ranks);
        CPU tensors or native=False: torch autograd + MpiAdam, in the parameters' dtype.
"""
import math
import os
import time
from collections import deque

import torch

from .rollout import add_vtarg_and_adv, flatten_segment, pipelined_segment_generator, traj_segment_generator
from .trpo import POL_KEYS, VF_KEYS, MpiAdam, TrpoLearner, _world, allmean, explained_variance, flat

LOSS_NAMES = ("pol_surr", "pol_entpen", "vf_loss", "kl", "ent")
NLOSS = 6                                       # LOSS_NAMES + clipfrac (the fraction of rows with |ratio - 1| > clip)
AC = 28
_HALF_LOG_2PI_E = 0.5 * math.log(2.0 * math.pi * math.e)
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def _neglogp(x, mean, logstd):
    """DiagGaussianPd.neglogp (src/distributions.py)"""
    return 0.5 * (((x - mean) / torch.exp(logstd)) ** 2).sum(-1) + _HALF_LOG_2PI * x.shape[-1] + logstd.sum(-1)


class PpoLearner:
    """One PPO update per segment: ppo1's `learn()` body between `seg_gen.__next__()` and the logging.  `update(seg)` -> stats, like
    TrpoLearner.update.  The schedule reads `timesteps_so_far`, which the driving loop sets before each update."""

    def __init__(self, pi, *, clip_param=0.2, entcoeff=0.0, optim_epochs=10, optim_stepsize=3e-4, optim_batchsize=64, gamma=0.99, lam=0.95,
                 adam_epsilon=1e-5, schedule="linear", max_timesteps=0, group=None, seed=0, native=None, per_minibatch=False):
        if schedule not in ("constant", "linear"):
            raise ValueError("schedule must be 'constant' or 'linear'")
        if schedule == "linear" and not max_timesteps:
            raise ValueError("schedule='linear' needs max_timesteps")
        self.pi = pi
        self.clip_param, self.entcoeff = float(clip_param), float(entcoeff)
        self.optim_epochs, self.optim_stepsize, self.optim_batchsize = int(optim_epochs), float(optim_stepsize), optim_batchsize
        self.gamma, self.lam, self.adam_epsilon = gamma, lam, adam_epsilon
        self.schedule, self.max_timesteps = schedule, max_timesteps
        self.group = group
        self.native = native                 # None: the kernels when they can run; False: torch autograd; True: the kernels or an error
        self.per_minibatch = per_minibatch   # True: dm_ppo_lossgrad + MpiAdam per minibatch even in one process
        self.timesteps_so_far = 0
        for k in POL_KEYS + VF_KEYS:
            pi.params[k].requires_grad_(True)
        self.pol = [pi.params[k] for k in POL_KEYS]
        self.vf = [pi.params[k] for k in VF_KEYS]
        self.adam = MpiAdam(self.pol + self.vf, epsilon=adam_epsilon, group=group)     # one step count for both nets
        self._perm_gen = torch.Generator(device=pi.device)
        self._perm_gen.manual_seed(int(seed))
        self.perm_source = None              # tests: callable(n) -> index tensor replacing the shuffles of Dataset (one per epoch, then the loss pass)
        self._scratch = None
        self._pg_scratch = None
        self.adam.sync()

    def lrmult(self):
        if self.schedule == "constant":
            return 1.0
        return max(1.0 - float(self.timesteps_so_far) / float(self.max_timesteps), 0.0)

    # ---- which path ----------------------------------------------------------------------------------------------------------
    def _native_ready(self, ob, ac):
        if self.native is False or ob.device.type != "cuda":
            return False
        p = self.pi.params
        ok = (ob.dtype == torch.float32 and ob.dim() == 2 and ob.shape[1] == 56 and ac.dtype == torch.float32 and ac.dim() == 2 and ac.shape[1] == AC
              and getattr(self.pi, "native", False) and tuple(p["polfc1/w"].shape) == (56, 100) and tuple(p["polfc2/w"].shape) == (100, 100)
              and tuple(p["polfinal/w"].shape) == (100, AC) and p["logstd"].numel() == AC and tuple(p["vffc1/w"].shape) == (56, 100)
              and tuple(p["vffc2/w"].shape) == (100, 100) and tuple(p["vffinal/w"].shape) == (100, 1)
              and all(p[k].dtype == torch.float32 for k in POL_KEYS + VF_KEYS) and tuple(self.pi.ob_rms.shape) == (56,))
        if not ok and self.native is True:
            raise ValueError("the PPO kernels need float32 [n, 56] observations / [n, 28] actions and the 56-100-100-28 policy with the 56-100-100-1 "
                             "value net on a GPU")
        return ok

    # ---- the kernels (dm_ppo_*) ------------------------------------------------------------------------------------------------
    def _lib(self):
        from . import _abi as A
        return A, A.load()

    def _stream(self, dev):
        import ctypes as C
        return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def _reserve(self, bs, dev):
        A, L = self._lib()
        need = int(L.dm_ppo_scratch_bytes(int(max(1, bs))))
        if self._scratch is None or self._scratch.numel() < need or self._scratch.device != dev:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._scratch

    def _rows(self, D):
        return [D[k] for k in ("ob", "ac", "atarg", "old_mean", "old_logstd", "ret")]

    def kernel_lossgrad(self, D, idx, theta, clip, grad=True):
        """dm_ppo_lossgrad on rows idx (int32 device tensor, or None: all rows) -> (losses [NLOSS] float64, flat gradient [pol + vf] or None)."""
        import ctypes as C
        A, L = self._lib()
        dev = D["ob"].device
        n = int(idx.numel()) if idx is not None else int(D["ob"].shape[0])
        sc = self._reserve(n if grad else 1, dev)
        out = torch.empty(NLOSS, dtype=torch.float64, device=dev)
        g = torch.empty(theta.numel(), dtype=torch.float32, device=dev) if grad else None
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        A.check(L.dm_ppo_lossgrad(*[p(t) for t in self._rows(D)], p(idx), n, p(theta), p(self.pi.ob_rms.mean), p(self.pi.ob_rms.std), float(clip),
                                  float(self.entcoeff), p(g), p(out), p(sc), sc.numel(), self._stream(dev)), L)
        return out, g

    def kernel_fit(self, D, idx, bs, theta, m, v, scales, clips):
        """dm_ppo_fit: len(scales) minibatches of bs rows idx [iters * bs] (int32 device) -> losses [iters, NLOSS] float64 on the device."""
        import ctypes as C
        A, L = self._lib()
        dev = D["ob"].device
        iters = len(scales)
        sc = self._reserve(bs, dev)
        out = torch.empty((iters, NLOSS), dtype=torch.float64, device=dev)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        A.check(L.dm_ppo_fit(*[p(t) for t in self._rows(D)], p(idx), iters, int(bs), p(theta), p(m), p(v), (C.c_float * iters)(*scales),
                             (C.c_float * iters)(*clips), float(self.adam.beta1), float(self.adam.beta2), float(self.adam.epsilon), float(self.entcoeff),
                             p(self.pi.ob_rms.mean), p(self.pi.ob_rms.std), p(out), p(sc), sc.numel(), self._stream(dev)), L)
        return out

    def _kernel_old_mean(self, ob, ac, atarg, old_logstd):
        """assign_old_eq_new as one dm_pg_losses launch with write_old = 1 (the kernel writes the policy's mean of every row)."""
        import ctypes as C
        A, L = self._lib()
        dev = ob.device
        if self._pg_scratch is None or self._pg_scratch.device != dev:
            self._pg_scratch = torch.empty(int(L.dm_pg_scratch_bytes()), dtype=torch.uint8, device=dev)
        old_mean = torch.empty((ob.shape[0], AC), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        theta = flat([t.detach() for t in self.pol]).contiguous()
        p = lambda t: C.c_void_p(t.data_ptr())
        A.check(L.dm_pg_losses(p(ob), int(ob.shape[0]), p(ac), p(atarg), p(old_mean), p(old_logstd), 1, p(theta), p(self.pi.ob_rms.mean),
                               p(self.pi.ob_rms.std), 0.0, 0, None, p(out), p(self._pg_scratch), self._stream(dev), 0), L)
        return old_mean

    # ---- torch autograd ----------------------------------------------------------------------------------------------------------
    def _z(self, ob):
        dt = self.pi.params["polfc1/w"].dtype
        rms = self.pi.ob_rms
        return torch.clamp((ob.to(dt) - rms.mean.to(dt)) / rms.std.to(dt), -5.0, 5.0)

    def torch_lossgrad(self, D, rows, clip, grad=True):
        """The losses of rows (a long tensor, or None: all rows) and, with grad, the flat gradient of pol_surr + pol_entpen + vf_loss by
        autograd, in the parameters' dtype -> (losses [NLOSS] float64, gradient or None)."""
        pi = self.pi
        sel = (lambda t: t) if rows is None else (lambda t: t.index_select(0, rows))
        ob, ac, A, old_mean, ret = sel(D["ob"]), sel(D["ac"]), sel(D["atarg"]), sel(D["old_mean"]), sel(D["ret"])
        dt = pi.params["polfc1/w"].dtype
        with torch.enable_grad() if grad else torch.no_grad():
            z = self._z(ob)
            mean, vpred = pi.forward_mean(ob, z), pi.forward_value(ob, z)
            logstd = pi.params["logstd"].reshape(-1)
            old_logstd = D["old_logstd"].to(dt)
            ac, A, old_mean, ret = ac.to(dt), A.to(dt), old_mean.to(dt), ret.to(dt)
            ratio = torch.exp(_neglogp(ac, old_mean, old_logstd) - _neglogp(ac, mean, logstd))
            surr1 = ratio * A
            surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * A
            pol_surr = -torch.where(surr1 <= surr2, surr1, surr2).mean()       # (the gradient flows to surr1 on a tie, like TF's minimum)
            ent = (logstd + _HALF_LOG_2PI_E).sum()
            pol_entpen = -self.entcoeff * ent
            vf_loss = ((vpred - ret) ** 2).mean()
            kl = TrpoLearner._kl(old_mean, old_logstd, mean, logstd).mean()
            clipfrac = ((ratio - 1.0).abs() > clip).to(dt).mean()
            g = flat(torch.autograd.grad(pol_surr + pol_entpen + vf_loss, self.pol + self.vf)) if grad else None
        losses = torch.stack([x.detach().reshape(()) for x in (pol_surr, pol_entpen, vf_loss, kl, ent, clipfrac)]).to(torch.float64)
        return losses, g

    # ---- one update ----------------------------------------------------------------------------------------------------------------
    def _perm(self, n, dev):
        if self.perm_source is not None:
            return self.perm_source(n).to(dev)
        return torch.randperm(n, device=dev, generator=self._perm_gen)

    def update(self, seg):
        add_vtarg_and_adv(seg, self.gamma, self.lam)
        fl = flatten_segment(seg)
        return self.update_batch(fl["ob"], fl["ac"], fl["adv"], fl["tdlamret"], fl["vpred"])

    def update_batch(self, ob, ac, adv, tdlamret, vpredbefore):
        """One update on the flat batch (rows of the segment): the whole of ppo1's update after add_vtarg_and_adv."""
        pi = self.pi
        dev = ob.device
        n = int(ob.shape[0])
        lrmult = self.lrmult()
        clip, stepsize = self.clip_param * lrmult, self.optim_stepsize * lrmult
        bs = int(self.optim_batchsize or n)
        nb = n // bs                                                        # Dataset.iterate_once: the final partial batch is dropped
        native = self._native_ready(ob, ac)
        fused = native and not self.per_minibatch and _world(self.group) == 1
        atarg = (adv - adv.mean()) / adv.std(unbiased=False)
        if native:
            ob = ob.contiguous(); ac = ac.contiguous()
            atarg = atarg.to(torch.float32).contiguous(); tdlamret = tdlamret.to(torch.float32).contiguous()
        TrpoLearner._rms_update(self, ob)                                   # pi.ob_rms.update(ob): once, before any step
        old_logstd = pi.params["logstd"].detach().reshape(-1).clone()
        if native:
            old_mean = self._kernel_old_mean(ob, ac, atarg, old_logstd)
        else:
            with torch.no_grad():
                old_mean = pi.forward_mean(ob, self._z(ob))
        D = dict(ob=ob, ac=ac, atarg=atarg, old_mean=old_mean, old_logstd=old_logstd, ret=tdlamret)
        ad = self.adam
        theta = ad.getflat().to(torch.float32).contiguous() if fused else None
        for _ in range(self.optim_epochs):
            perm = self._perm(n, dev)
            if nb == 0:
                continue
            if fused:
                idx = perm[:nb * bs].to(torch.int32).contiguous()
                scales = [stepsize * math.sqrt(1 - ad.beta2 ** (ad.t + 1 + k)) / (1 - ad.beta1 ** (ad.t + 1 + k)) for k in range(nb)]
                self.kernel_fit(D, idx, bs, theta, ad.m, ad.v, scales, [clip] * nb)
                ad.t += nb
                continue
            for k in range(nb):
                rows = perm[k * bs:(k + 1) * bs]
                if native:
                    _, g = self.kernel_lossgrad(D, rows.to(torch.int32).contiguous(), ad.getflat().to(torch.float32).contiguous(), clip)
                else:
                    _, g = self.torch_lossgrad(D, rows, clip)
                ad.update(g, stepsize)
        if fused:
            ad.setfromflat(theta)
        # the losses: one more shuffled pass over the full minibatches, no step
        perm = self._perm(n, dev)
        if nb == 0:
            losses = torch.full((NLOSS,), float("nan"), dtype=torch.float64, device=dev)
        elif native:
            losses, _ = self.kernel_lossgrad(D, perm[:nb * bs].to(torch.int32).contiguous(), ad.getflat().to(torch.float32).contiguous(), clip, grad=False)
        else:
            losses, _ = self.torch_lossgrad(D, perm[:nb * bs], clip, grad=False)
        losses = allmean(losses, self.group).tolist()
        pi.mark_dirty()                                                     # parameters / obs filter changed in place: the native act() repacks
        stats = {"loss_" + k: v for k, v in zip(LOSS_NAMES, losses)}
        stats.update(clipfrac=losses[5], lrmult=lrmult, optim_steps=nb * self.optim_epochs,
                     ev_tdlam_before=explained_variance(vpredbefore.to(tdlamret.dtype), tdlamret))
        return stats


def learn(env, pi, *, timesteps_per_batch=2048, max_iters=0, max_timesteps=0, max_seconds=0, callback=None, log=print, group=None, log_dir=None,
          fused=None, schedule="linear", **learner_kwargs):
    """ppo1's `learn()` over a DPVecEnv (autoreset="init"; or a list of them: pipelined rollouts) and an MlpPolicy, with trpo.learn's loop,
    stopping rules (`max_iters`, `max_timesteps` env steps (global), `max_seconds`), multi-rank handling and output files (`log_dir`: rank 0
    writes progress.csv and monitor.csv).  Episode statistics over ppo1's window of the last 100 episodes.  schedule="linear" needs
    max_timesteps.  fused: the rollout's policy step inside the env step kernel (None: when possible).  Returns the per-iteration stats:
    loss_pol_surr, loss_pol_entpen, loss_vf_loss, loss_kl, loss_ent, clipfrac, ev_tdlam_before, EpLenMean, EpRewMean, EpThisIter, ..."""
    import torch.distributed as dist
    assert sum([max_iters > 0, max_timesteps > 0, max_seconds > 0]) >= 1
    learner = PpoLearner(pi, group=group, schedule=schedule, max_timesteps=max_timesteps, **learner_kwargs)
    if isinstance(env, (list, tuple)):
        seg_gen = pipelined_segment_generator(pi, list(env), timesteps_per_batch, stochastic=True)
        n_envs_local = sum(e.num_envs for e in env)
    else:
        from .rollout import can_fuse
        use_fused = can_fuse(pi, env) if fused is None else bool(fused)
        seg_gen = traj_segment_generator(pi, env, timesteps_per_batch, stochastic=True, fused=use_fused)
        n_envs_local = env.num_envs
    world = _world(group)
    rank = dist.get_rank(group) if world > 1 else 0
    episodes_so_far = timesteps_so_far = iters_so_far = 0
    tstart = time.time()
    lenbuffer, rewbuffer = deque(maxlen=100), deque(maxlen=100)
    history = []
    progress = monitor = None
    if log_dir and rank == 0:
        from .logio import ProgressCsv, MonitorWriter
        os.makedirs(log_dir, exist_ok=True)
        progress = ProgressCsv(os.path.join(log_dir, "progress.csv"))
        monitor = MonitorWriter(os.path.join(log_dir, "monitor.json"), t_start=tstart)
    while True:
        if callback:
            callback(locals(), globals())
        if max_timesteps and timesteps_so_far >= max_timesteps:
            break
        if max_iters and iters_so_far >= max_iters:
            break
        if max_seconds:
            stop = time.time() - tstart >= max_seconds                  # decided collectively, as trpo.learn does
            if world > 1:
                flag = torch.tensor([1.0 if stop else 0.0], dtype=torch.float32, device=pi.device)
                dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
                stop = bool(flag.item() > 0)
            if stop:
                break
        seg = next(seg_gen)
        learner.timesteps_so_far = timesteps_so_far
        stats = learner.update(seg)
        if getattr(seg, "info", None):
            stats["rollout"] = dict(seg.info)
        lens, rets = seg["ep_lens"], seg["ep_rets"]
        n_eps = torch.tensor([len(lens), sum(lens), sum(rets)], dtype=torch.float64, device=pi.device)
        if world > 1:
            dist.all_reduce(n_eps, group=group)
        lenbuffer.extend(lens[-100:]); rewbuffer.extend(rets[-100:])
        episodes_so_far += int(n_eps[0]); timesteps_so_far += timesteps_per_batch * n_envs_local * world
        iters_so_far += 1
        stats.update(EpLenMean=float(sum(lenbuffer) / max(1, len(lenbuffer))), EpRewMean=float(sum(rewbuffer) / max(1, len(rewbuffer))),
                     EpLenMeanIter=float(n_eps[1] / max(1.0, float(n_eps[0]))), EpThisIter=int(n_eps[0]), EpisodesSoFar=episodes_so_far,
                     TimestepsSoFar=timesteps_so_far, TimeElapsed=time.time() - tstart, iteration=iters_so_far)
        history.append(stats)
        if progress is not None:
            progress.writekvs({k: stats.get(k) for k in ("loss_pol_surr", "loss_pol_entpen", "loss_vf_loss", "loss_kl", "loss_ent", "clipfrac",
                                                        "ev_tdlam_before", "EpLenMean", "EpRewMean", "EpThisIter", "EpisodesSoFar",
                                                        "TimestepsSoFar", "TimeElapsed")})
            monitor.write_episodes(rets, lens)
        if log and rank == 0:
            log("iter %4d  steps %10d  eps %7d  EpLenMean %7.1f  (this iter %7.1f)  pol_surr %+.4f  vf_loss %.4f  kl %.5f  clipfrac %.3f  ent %6.2f  "
                "ev %.3f  %.1fs" % (iters_so_far, timesteps_so_far, stats["EpThisIter"], stats["EpLenMean"], stats["EpLenMeanIter"],
                                    stats["loss_pol_surr"], stats["loss_vf_loss"], stats["loss_kl"], stats["clipfrac"], stats["loss_ent"],
                                    stats["ev_tdlam_before"], stats["TimeElapsed"]))
    if progress is not None:
        progress.close(); monitor.close()
    return history
