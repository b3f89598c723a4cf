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
import torch

from . import _abi
from .rollout import add_vtarg_and_adv, flatten_segment
from .trpo import _HALF_LOG_2PI_E, POL_KEYS, VF_KEYS, MpiAdam, TrpoLearner, _neglogp, _world, allmean, explained_variance, flat, native_nets, rms_update

LOSS_NAMES = ("pol_surr", "pol_entpen", "vf_loss", "kl", "ent")
NLOSS = 6                                       # LOSS_NAMES + clipfrac (the fraction of rows with |ratio - 1| > clip)
AC = 28


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
        self._rms_scratch = None
        self.adam.sync()

    def lrmult(self):
        if self.schedule == "constant":
            return 1.0
        return max(1.0 - float(self.timesteps_so_far) / float(self.max_timesteps), 0.0)

    # ---- which path ----------------------------------------------------------------------------------------------------------
    def _native_ready(self, ob, ac):
        if self.native is False or ob.device.type != "cuda":
            return False
        ok = (ob.dtype == torch.float32 and ob.dim() == 2 and ob.shape[1] == 56 and ac.dtype == torch.float32 and ac.dim() == 2 and ac.shape[1] == AC
              and native_nets(self.pi, POL_KEYS + VF_KEYS))
        if not ok and self.native is True:
            raise ValueError("the PPO kernels need float32 [n, 56] observations / [n, 28] actions and the 56-100-100-28 policy with the 56-100-100-1 "
                             "value net on a GPU")
        return ok

    # ---- the kernels (dm_ppo_*) ------------------------------------------------------------------------------------------------
    def _reserve(self, bs, dev):
        self._scratch = _abi.scratch(self._scratch, _abi.load().dm_ppo_scratch_bytes(int(max(1, bs))), dev)
        return self._scratch

    def _rows(self, D):
        return [D[k] for k in ("ob", "ac", "atarg", "old_mean", "old_logstd", "ret")]

    def kernel_lossgrad(self, D, idx, theta, clip, grad=True):
        """dm_ppo_lossgrad on rows idx (int32 device tensor, or None: all rows) -> (losses [NLOSS] float64, flat gradient [pol + vf] or None)."""
        L, p = _abi.load(), _abi.ptr
        dev = D["ob"].device
        n = int(idx.numel()) if idx is not None else int(D["ob"].shape[0])
        sc = self._reserve(n if grad else 1, dev)
        out = torch.empty(NLOSS, dtype=torch.float64, device=dev)
        g = torch.empty(theta.numel(), dtype=torch.float32, device=dev) if grad else None
        _abi.check(L.dm_ppo_lossgrad(*[p(t) for t in self._rows(D)], p(idx), n, p(theta), p(self.pi.ob_rms.mean), p(self.pi.ob_rms.std), float(clip),
                                     float(self.entcoeff), p(g), p(out), p(sc), sc.numel(), _abi.stream(dev)), L)
        return out, g

    def kernel_fit(self, D, idx, bs, theta, m, v, scales, clips):
        """dm_ppo_fit: len(scales) minibatches of bs rows idx [iters * bs] (int32 device) -> losses [iters, NLOSS] float64 on the device."""
        import ctypes as C
        L, p = _abi.load(), _abi.ptr
        dev = D["ob"].device
        iters = len(scales)
        sc = self._reserve(bs, dev)
        out = torch.empty((iters, NLOSS), dtype=torch.float64, device=dev)
        _abi.check(L.dm_ppo_fit(*[p(t) for t in self._rows(D)], p(idx), iters, int(bs), p(theta), p(m), p(v), (C.c_float * iters)(*scales),
                                (C.c_float * iters)(*clips), float(self.adam.beta1), float(self.adam.beta2), float(self.adam.epsilon), float(self.entcoeff),
                                p(self.pi.ob_rms.mean), p(self.pi.ob_rms.std), p(out), p(sc), sc.numel(), _abi.stream(dev)), L)
        return out

    def _kernel_old_mean(self, ob, ac, atarg, old_logstd):
        """assign_old_eq_new as one dm_pg_losses launch with write_old = 1 (the kernel writes the policy's mean of every row)."""
        L, p = _abi.load(), _abi.ptr
        dev = ob.device
        self._pg_scratch = _abi.scratch(self._pg_scratch, L.dm_pg_scratch_bytes(), dev)
        old_mean = torch.empty((ob.shape[0], AC), dtype=torch.float32, device=dev)
        out = torch.empty(2, dtype=torch.float64, device=dev)
        theta = flat([t.detach() for t in self.pol]).contiguous()
        _abi.check(L.dm_pg_losses(p(ob), int(ob.shape[0]), p(ac), p(atarg), p(old_mean), p(old_logstd), 1, p(theta), p(self.pi.ob_rms.mean),
                                  p(self.pi.ob_rms.std), 0.0, 0, None, p(out), p(self._pg_scratch), _abi.stream(dev), 0), L)
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
        rms_update(pi, ob, self.group, self)                                # pi.ob_rms.update(ob): once, before any step
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
                self.kernel_fit(D, idx, bs, theta, ad.m, ad.v, ad.stepsizes(stepsize, nb), [clip] * nb)
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
          fused=None, schedule="linear", bootstrap_time_limit=False, log_reward_terms=False, **learner_kwargs):
    """ppo1's `learn()` over a DPVecEnv (autoreset="init"; or a list of them: pipelined rollouts) and an MlpPolicy, with trpo.learn's loop (train_loop.run),
    stopping rules (`max_iters`, `max_timesteps` env steps (global), `max_seconds`), multi-rank handling and output files (`log_dir`: rank 0
    writes progress.csv and monitor.csv).  Episode statistics over ppo1's window of the last 100 episodes.  schedule="linear" needs
    max_timesteps.  fused: the rollout's policy step inside the env step kernel (None: when possible).  Returns the per-iteration stats:
    loss_pol_surr, loss_pol_entpen, loss_vf_loss, loss_kl, loss_ent, clipfrac, ev_tdlam_before, EpLenMean, EpRewMean, EpThisIter, ...
    bootstrap_time_limit: as in trpo.learn (value bootstrap where the time limit ends an episode; adds TruncThisIter).
    log_reward_terms: as in trpo.learn (adds ErrPose, ErrVel, ErrEndEff, ErrRoot, ErrCom after the keys above; off: keys and columns unchanged)."""
    from . import train_loop
    assert sum([max_iters > 0, max_timesteps > 0, max_seconds > 0]) >= 1
    learner = PpoLearner(pi, group=group, schedule=schedule, max_timesteps=max_timesteps, **learner_kwargs)
    seg_gen, n_envs_local = train_loop.segments(pi, env, timesteps_per_batch, fused, bootstrap_time_limit, log_reward_terms)
    steps_per_iter = timesteps_per_batch * n_envs_local * _world(group)

    def iterate(timesteps_so_far):
        seg = next(seg_gen)
        learner.timesteps_so_far = timesteps_so_far
        stats = learner.update(seg)
        if getattr(seg, "info", None):
            stats["rollout"] = dict(seg.info)
        lens, rets = seg["ep_lens"], seg["ep_rets"]
        train_loop.truncation_stat(stats, seg)
        train_loop.reward_terms_stat(stats, seg, group)
        return stats, {"EpLenMean": lens, "EpRewMean": rets}, [(rets, lens)], steps_per_iter

    def log_line(stats):
        return ("iter %4d  steps %10d  eps %7d  EpLenMean %7.1f  (this iter %7.1f)  pol_surr %+.4f  vf_loss %.4f  kl %.5f  clipfrac %.3f  ent %6.2f  "
                "ev %.3f  %.1fs" % (stats["iteration"], stats["TimestepsSoFar"], stats["EpThisIter"], stats["EpLenMean"], stats["EpLenMeanIter"],
                                    stats["loss_pol_surr"], stats["loss_vf_loss"], stats["loss_kl"], stats["clipfrac"], stats["loss_ent"],
                                    stats["ev_tdlam_before"], stats["TimeElapsed"]))

    return train_loop.run(pi, iterate, window=100, log_line=log_line, names=locals(), max_iters=max_iters, max_timesteps=max_timesteps,
                          max_seconds=max_seconds, callback=callback, log=log, group=group, log_dir=log_dir,
                          columns=("loss_pol_surr", "loss_pol_entpen", "loss_vf_loss", "loss_kl", "loss_ent", "clipfrac", "ev_tdlam_before",
                                   "EpLenMean", "EpRewMean", "EpThisIter", "EpisodesSoFar", "TimestepsSoFar", "TimeElapsed")
                          + (train_loop.ERR_KEYS if log_reward_terms else ()))
