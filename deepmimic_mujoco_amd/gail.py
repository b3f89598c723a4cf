"""GAIL: the reference's second learner (src/gail.py, src/adversary.py, src/utils/mujoco_dset.py) over the device-resident rollout.

    TransitionClassifier  the discriminator D(ob, ac) of src/adversary.py: parameters on the device, its own obs filter, the policy's reward
                          for a whole segment in one launch (dm_disc_reward) and the loss + flat gradient in two (dm_disc_lossgrad,
                          csrc/disc_kernel.h); a torch-autograd path where the kernels cannot run (CPU tensors, other network sizes)
    ExpertDataset         Mujoco_Dset / Dset: the expert's (ob, ac) transitions on the device, batches gathered by index in the reference's
                          shuffle order (its own seeded numpy generator)
    learn                 src/gail.py:112-343: g_step TRPO updates on segments rewarded by D (trpo.TrpoLearner), then the D update
"""
import math
import os

import numpy as np
import torch

from . import _abi as A
from .policy import RunningMeanStd
from .trpo import MpiAdam, TrpoLearner

# adversary.py `get_trainable_variables()` order (tf.contrib.layers.fully_connected scopes)
ADV_KEYS = ("fully_connected/weights", "fully_connected/biases", "fully_connected_1/weights", "fully_connected_1/biases",
            "fully_connected_2/weights", "fully_connected_2/biases")
LOSS_NAMES = ("generator_loss", "expert_loss", "entropy", "entropy_loss", "generator_acc", "expert_acc")   # adversary.py `loss_name`


def _logit_bernoulli_entropy(x):
    """adversary.py: (1 - sigmoid(x)) x - logsigmoid(x) = (1 - sigmoid(x)) x + softplus(-x)."""
    return (1.0 - torch.sigmoid(x)) * x + torch.nn.functional.softplus(-x)


def _sigmoid_ce(x, z):
    """tf.nn.sigmoid_cross_entropy_with_logits: max(x, 0) - x z + log1p(exp(-|x|))."""
    return torch.clamp(x, min=0.0) - x * z + torch.log1p(torch.exp(-torch.abs(x)))


class TransitionClassifier:
    """src/adversary.py TransitionClassifier with hidden_size units: concat((ob - rms.mean) / rms.std, ac) -> tanh -> tanh -> logit, fp32.
    `theta` is ONE flat float32 leaf tensor in the reference's variable order (W1 [ob+ac, h], b1, W2 [h, h], b2, w3 [h, 1], b3), initialised
    as TF's defaults do (Glorot-uniform weights, zero biases); `obs_rms` is the adversary's own filter (scope adversary/obfilter).
    native: None = the kernels whenever they can run (CUDA tensors, the reference's 56 + 28 -> 100 -> 100 -> 1 network), False = torch."""

    def __init__(self, ob_dim=56, ac_dim=28, hidden_size=100, entcoeff=1e-3, device="cpu", seed=0, native=None):
        self.ob_dim, self.ac_dim, self.hidden_size, self.entcoeff = int(ob_dim), int(ac_dim), int(hidden_size), float(entcoeff)
        self.device = torch.device(device)
        self.loss_name = list(LOSS_NAMES)
        i, h = self.ob_dim + self.ac_dim, self.hidden_size
        self.shapes = [(i, h), (h,), (h, h), (h,), (h, 1), (1,)]
        gen = torch.Generator().manual_seed(int(seed))
        parts = []
        for shp in self.shapes:
            if len(shp) == 2:        # glorot_uniform: U(-l, l), l = sqrt(6 / (fan_in + fan_out))
                lim = math.sqrt(6.0 / (shp[0] + shp[1]))
                parts.append((torch.rand(shp, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * lim)
            else:
                parts.append(torch.zeros(shp, dtype=torch.float32))
        self.theta = torch.cat([p.reshape(-1) for p in parts]).to(self.device).contiguous()
        self.obs_rms = RunningMeanStd(self.ob_dim, device=self.device)
        self.native = native
        self._scratch = None

    # ---- parameters -----------------------------------------------------------------------------------------------------------
    def get_trainable_variables(self):
        return [self.theta]

    def unflatten(self, theta=None):
        theta = self.theta if theta is None else theta
        out, o = [], 0
        for shp in self.shapes:
            n = int(np.prod(shp))
            out.append(theta[o:o + n].reshape(shp)); o += n
        return out

    def state_dict(self):
        """The adversary's variables with the reference's names (scope `adversary/`), the filter's float64 sums and count."""
        d = {"adversary/" + k: v.detach().cpu().numpy().copy() for k, v in zip(ADV_KEYS, self.unflatten())}
        d["adversary/obfilter/runningsum"] = self.obs_rms.sum.cpu().numpy()
        d["adversary/obfilter/runningsumsq"] = self.obs_rms.sumsq.cpu().numpy()
        d["adversary/obfilter/count"] = self.obs_rms.count.cpu().numpy()
        return d

    def load_state_dict(self, d):
        parts = []
        for k, shp in zip(ADV_KEYS, self.shapes):
            v = np.asarray(d["adversary/" + k], dtype=np.float32)
            if tuple(v.shape) != tuple(shp):
                raise ValueError("adversary/%s: shape %s != %s" % (k, v.shape, shp))
            parts.append(v.reshape(-1))
        with torch.no_grad():
            self.theta.copy_(torch.from_numpy(np.concatenate(parts)).to(self.device))
        self.obs_rms.sum = torch.as_tensor(np.asarray(d["adversary/obfilter/runningsum"]), dtype=torch.float64).to(self.device)
        self.obs_rms.sumsq = torch.as_tensor(np.asarray(d["adversary/obfilter/runningsumsq"]), dtype=torch.float64).to(self.device)
        self.obs_rms.count = torch.as_tensor(np.asarray(d["adversary/obfilter/count"]), dtype=torch.float64).to(self.device)
        self.obs_rms._refresh()
        return self

    def save_npz(self, path):
        np.savez(path, **self.state_dict())

    @classmethod
    def from_npz(cls, path, device="cpu", **kw):
        d = dict(np.load(path))
        w1 = d["adversary/fully_connected/weights"]
        rg = cls(ob_dim=d["adversary/obfilter/runningsum"].shape[0], ac_dim=w1.shape[0] - d["adversary/obfilter/runningsum"].shape[0],
                 hidden_size=w1.shape[1], device=device, **kw)
        return rg.load_state_dict(d)

    # ---- the kernels ----------------------------------------------------------------------------------------------------------
    def _native_ok(self, *xs):
        if self.native is False or self.device.type != "cuda" or (self.ob_dim, self.ac_dim, self.hidden_size) != (56, 28, 100):
            return False
        return all(x.is_cuda and x.device == self.device for x in xs)

    # ---- forward (torch) ------------------------------------------------------------------------------------------------------
    def logits(self, ob, ac, theta=None):
        """The network of adversary.py build_graph in float32 torch ops: [n] logits."""
        w1, b1, w2, b2, w3, b3 = self.unflatten(theta)
        obz = (ob.to(torch.float32) - self.obs_rms.mean) / self.obs_rms.std
        x = torch.cat([obz, ac.to(torch.float32)], -1)
        h1 = torch.tanh(x @ w1 + b1)
        h2 = torch.tanh(h1 @ w2 + b2)
        return (h2 @ w3 + b3)[..., 0]

    @staticmethod
    def reward_of_logits(x):
        """adversary.py `reward_op` literally, in fp32: saturates at -log(1e-8) ~ 18.42 once sigmoid rounds to 1 (NOT softplus(x))."""
        return -torch.log(1.0 - torch.sigmoid(x.to(torch.float32)) + 1e-8)

    def reward_into(self, ob64, ac64, out64):
        """D's reward of every row: ob64 [..., 56] / ac64 [..., 28] float64, out64 [...] float64 (one launch of dm_disc_reward on the
        current stream when the kernels can run)."""
        n = out64.numel()
        if (self._native_ok(ob64, ac64, out64) and ob64.dtype == torch.float64 and ac64.dtype == torch.float64 and out64.dtype == torch.float64
                and ob64.is_contiguous() and ac64.is_contiguous() and out64.is_contiguous() and ob64.numel() == 56 * n and ac64.numel() == 28 * n):
            L, p = A.load(), A.ptr
            A.check(L.dm_disc_reward(p(self.theta), p(self.obs_rms.mean), p(self.obs_rms.std), p(ob64), p(ac64), int(n), p(out64), A.stream(self.device)), L)
            return out64
        with torch.no_grad():
            r = self.reward_of_logits(self.logits(ob64.reshape(-1, self.ob_dim), ac64.reshape(-1, self.ac_dim)))
        out64.copy_(r.to(torch.float64).reshape(out64.shape))
        return out64

    def get_reward(self, obs, acs):
        """adversary.py get_reward: [n, 1] float32 rewards of a batch (a single ob / ac is a batch of one)."""
        ob = torch.as_tensor(np.asarray(obs) if not torch.is_tensor(obs) else obs, device=self.device).to(torch.float64)
        ac = torch.as_tensor(np.asarray(acs) if not torch.is_tensor(acs) else acs, device=self.device).to(torch.float64)
        ob = ob.reshape(-1, self.ob_dim).contiguous(); ac = ac.reshape(-1, self.ac_dim).contiguous()
        out = torch.empty(ob.shape[0], dtype=torch.float64, device=self.device)
        self.reward_into(ob, ac, out)
        return out.to(torch.float32)[:, None]

    # ---- loss and gradient ----------------------------------------------------------------------------------------------------
    def lossandgrad(self, g_ob, g_ac, e_ob, e_ac):
        """adversary.py `lossandgrad`: (losses [6] float64 in LOSS_NAMES order, flat gradient of the total loss [n_params] float32).
        Generator and expert batches may differ in size (an expert set smaller than the batch)."""
        ng, ne = int(g_ob.shape[0]), int(e_ob.shape[0])
        if ng < 1 or ne < 1:
            raise ValueError("lossandgrad needs at least one generator and one expert row (%d, %d)" % (ng, ne))
        if self._native_ok(g_ob, g_ac, e_ob, e_ac):
            L, p = A.load(), A.ptr
            f = lambda x, d: x.to(torch.float32).reshape(-1, d).contiguous()
            g_ob, g_ac, e_ob, e_ac = f(g_ob, 56), f(g_ac, 28), f(e_ob, 56), f(e_ac, 28)
            self._scratch = A.scratch(self._scratch, L.dm_disc_scratch_bytes(ng, ne), self.device)
            grad = torch.empty(self.theta.numel(), dtype=torch.float32, device=self.device)
            losses = torch.empty(6, dtype=torch.float64, device=self.device)
            A.check(L.dm_disc_lossgrad(p(self.theta), p(self.obs_rms.mean), p(self.obs_rms.std), p(g_ob), p(g_ac), ng, p(e_ob), p(e_ac), ne,
                                       self.entcoeff, p(grad), p(losses), p(self._scratch), self._scratch.numel(), A.stream(self.device)), L)
            return losses, grad
        return self._lossandgrad_torch(g_ob, g_ac, e_ob, e_ac)

    def _lossandgrad_torch(self, g_ob, g_ac, e_ob, e_ac):
        th = self.theta.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            xg = self.logits(g_ob, g_ac, th); xe = self.logits(e_ob, e_ac, th)
            gl = _sigmoid_ce(xg, 0.0).mean(); el = _sigmoid_ce(xe, 1.0).mean()
            ent = _logit_bernoulli_entropy(torch.cat([xg, xe])).mean()
            entl = -self.entcoeff * ent
            total = gl + el + entl
            (g,) = torch.autograd.grad(total, th)
        with torch.no_grad():
            gacc = (torch.sigmoid(xg) < 0.5).to(torch.float32).mean(); eacc = (torch.sigmoid(xe) > 0.5).to(torch.float32).mean()
            losses = torch.stack([gl, el, ent, entl, gacc, eacc]).detach().to(torch.float64)
        return losses, g.detach()


class _Index:
    """Dset (mujoco_dset.py) over row indices: `init_pointer` re-shuffles the set's CURRENT order, as the reference shuffles its arrays."""

    def __init__(self, order, randomize, rng):
        self.order, self.randomize, self.rng = np.asarray(order, dtype=np.int64), randomize, rng
        self.num_pairs = len(self.order)
        self.init_pointer()

    def init_pointer(self):
        self.pointer = 0
        if self.randomize:
            idx = np.arange(self.num_pairs)
            self.rng.shuffle(idx)
            self.order = self.order[idx]

    def next_indices(self, batch_size):
        if batch_size < 0:
            return self.order
        if self.pointer + batch_size >= self.num_pairs:
            self.init_pointer()
        end = self.pointer + batch_size
        out = self.order[self.pointer:end]
        self.pointer = end
        return out


class ExpertDataset:
    """src/utils/mujoco_dset.py Mujoco_Dset.  `expert` is a path to an .npz or a dict with `obs` / `acs` of shape (N, L, ...) or object
    arrays of N trajectories of unequal lengths, and `ep_rets` (the reader's key) or `rets` (what `trpo.py --save_sample` writes).
    The transitions live on `device` as float32; `get_next_batch(b)` gathers rows by index in Dset's order: when pointer + b >= the set's
    size the set is re-shuffled and restarts at 0, so the batch is SHORTER than b when the set is smaller than b.  The shuffles come from
    this dataset's own numpy generator (np.random.RandomState(seed)), drawn in the reference's order (dset, train_set, val_set at load)."""

    def __init__(self, expert, traj_limitation=-1, train_fraction=0.7, randomize=True, seed=0, device="cpu"):
        data = dict(np.load(expert, allow_pickle=True)) if isinstance(expert, (str, bytes, os.PathLike)) else dict(expert)
        if traj_limitation < 0:
            traj_limitation = len(data["obs"])
        obs, acs = data["obs"][:traj_limitation], data["acs"][:traj_limitation]
        if len(obs.shape[2:]) != 0:
            obs = np.reshape(obs, [-1, int(np.prod(obs.shape[2:]))]); acs = np.reshape(acs, [-1, int(np.prod(acs.shape[2:]))])
        else:                                                       # ragged: object arrays of (L_i, dim) trajectories
            obs = np.vstack(list(obs)); acs = np.vstack(list(acs))
        rets = data["ep_rets"] if "ep_rets" in data else data["rets"]
        self.rets = np.asarray(rets[:traj_limitation], dtype=np.float64).reshape(-1)
        self.avg_ret = float(self.rets.sum() / len(self.rets))
        self.std_ret = float(np.std(self.rets))
        if len(acs) > 2:
            acs = np.squeeze(acs)
        assert len(obs) == len(acs)
        self.num_traj = min(traj_limitation, len(data["obs"]))
        self.num_transition = len(obs)
        self.device = torch.device(device)
        self.obs = torch.as_tensor(np.asarray(obs, dtype=np.float32)).to(self.device)
        self.acs = torch.as_tensor(np.asarray(acs, dtype=np.float32)).reshape(self.num_transition, -1).to(self.device)
        self.rng = np.random.RandomState(seed)
        n, cut = self.num_transition, int(self.num_transition * train_fraction)
        self.dset = _Index(np.arange(n), randomize, self.rng)
        self.train_set = _Index(np.arange(cut), randomize, self.rng)           # (for behaviour cloning, as in the reference)
        self.val_set = _Index(np.arange(cut, n), randomize, self.rng)

    def next_indices(self, batch_size, split=None):
        s = {None: self.dset, "train": self.train_set, "val": self.val_set}.get(split)
        if s is None:
            raise NotImplementedError(split)
        return s.next_indices(batch_size)

    def get_next_batch(self, batch_size, split=None):
        idx = torch.from_numpy(np.ascontiguousarray(self.next_indices(int(batch_size), split))).to(self.device)
        return self.obs.index_select(0, idx), self.acs.index_select(0, idx)


def learn(env, pi, reward_giver, expert, *, g_step=3, d_step=1, d_stepsize=3e-4, timesteps_per_batch=1024, max_iters=0, max_timesteps=0,
          max_seconds=0, entcoeff=0.0, max_kl=0.01, cg_iters=10, cg_damping=0.1, gamma=0.995, lam=0.97, vf_iters=5, vf_stepsize=1e-3,
          callback=None, log=print, group=None, log_dir=None, fused=None, seed=0, algo="trpo", ppo_kwargs=None, bootstrap_time_limit=False,
          log_reward_terms=False, **learner_kwargs):
    """`learn()` of src/gail.py:112-343 (hyper-parameters as its `train()` passes them) over a DPVecEnv (autoreset="init") and an MlpPolicy.
    One iteration: g_step times a segment rewarded by `reward_giver` and a TRPO update on it (trpo.TrpoLearner), then the D update on the
    LAST segment's (ob, ac): one `expert.get_next_batch(len(ob))` whose result is dropped, then for each of the d_step minibatches of
    len(ob) // d_step rows (a shuffle of the segment, `dataset.iterbatches` without the final partial batch) an expert batch of the same
    size, the adversary's filter updated with both, the loss gradient all-mean'd into MpiAdam(d_stepsize).
    Episode statistics come from the last segment as in the reference (:345-357): EpRewMean averages D's returns, EpTrueRewMean the env's;
    TimestepsSoFar adds the lengths of the episodes that ended (:361).  Stops after max_iters iterations, max_timesteps or max_seconds.
    With `log_dir`, rank 0 writes progress.csv and monitor.csv (the env's returns of every finished episode) as trpo.learn does.
    algo="ppo" (the reference's --algo, src/gail.py:394): the G updates are ppo.PpoLearner's, with gamma, lam, entcoeff, seed and `ppo_kwargs`
    (its linear schedule over max_timesteps when that is the stopping rule, else a constant one); the TRPO arguments are then unused.
    bootstrap_time_limit: as in trpo.learn — the value bootstrap where the time limit ends an episode, on the discriminator's rewards like every other
    row; adds TruncThisIter (of the last segment, like the episode statistics).
    log_reward_terms (the env has reward="imitation"): as in trpo.learn — ErrPose, ErrVel, ErrEndEff, ErrRoot, ErrCom of the states the last segment ends in,
    after the keys above; off: keys and columns unchanged."""
    from . import train_loop
    assert sum([max_iters > 0, max_timesteps > 0, max_seconds > 0]) >= 1
    from .rollout import can_fuse, traj_segment_generator
    if algo == "trpo":
        learner = TrpoLearner(pi, max_kl=max_kl, cg_iters=cg_iters, cg_damping=cg_damping, gamma=gamma, lam=lam, entcoeff=entcoeff,
                              vf_iters=vf_iters, vf_stepsize=vf_stepsize, group=group, seed=seed, **learner_kwargs)
    elif algo == "ppo":
        from .ppo import PpoLearner
        kw = dict(schedule="linear" if max_timesteps else "constant", max_timesteps=max_timesteps)
        kw.update(ppo_kwargs or {})
        learner = PpoLearner(pi, gamma=gamma, lam=lam, entcoeff=entcoeff, group=group, seed=seed, **kw)
    else:
        raise ValueError("algo must be 'trpo' or 'ppo'")
    d_adam = MpiAdam(reward_giver.get_trainable_variables(), group=group)
    d_adam.sync()
    use_fused = can_fuse(pi, env) if fused is None else bool(fused)
    seg_gen = traj_segment_generator(pi, env, timesteps_per_batch, stochastic=True, fused=use_fused, reward_giver=reward_giver,
                                     bootstrap_time_limit=bootstrap_time_limit, reward_terms=log_reward_terms)
    d_gen = torch.Generator(device=pi.device)
    d_gen.manual_seed(int(seed) + 1)

    def iterate(timesteps_so_far):
        # ---- update G (:259-326) ----
        segs = []
        for _ in range(g_step):
            seg = next(seg_gen)
            learner.timesteps_so_far = timesteps_so_far                 # (PPO's schedule)
            stats = learner.update(seg)
            segs.append(seg)
        # ---- update D (:328-343) ----
        ob = seg["ob"].reshape(-1, seg["ob"].shape[-1]); ac = seg["ac"].reshape(-1, seg["ac"].shape[-1])
        n = ob.shape[0]
        expert.get_next_batch(n)
        bs = n // d_step
        inds = torch.randperm(n, device=ob.device, generator=d_gen)
        d_losses = []
        for k in range(d_step if bs > 0 else 0):
            idx = inds[k * bs:(k + 1) * bs]
            mbob, mbac = ob.index_select(0, idx), ac.index_select(0, idx)
            eob, eac = expert.get_next_batch(bs)
            eob, eac = eob.to(mbob.device), eac.to(mbob.device)
            reward_giver.obs_rms.update(torch.cat([mbob, eob], 0), group=group)
            losses, g = reward_giver.lossandgrad(mbob, mbac, eob, eac)
            d_adam.update(g, d_stepsize)                                    # (MpiAdam all-means the gradient first: the reference's allmean(g))
            d_losses.append(losses)
        d_mean = torch.stack(d_losses).mean(0).tolist() if d_losses else [float("nan")] * 6
        for name, val in zip(reward_giver.loss_name, d_mean):
            stats[name] = val
        # ---- episode statistics of the last segment (:345-364); the monitor file gets every segment's ----
        train_loop.truncation_stat(stats, seg)
        train_loop.reward_terms_stat(stats, seg, group)
        episodes = {"EpLenMean": list(seg["ep_lens"]), "EpRewMean": list(seg["ep_rets"]), "EpTrueRewMean": list(seg["ep_true_rets"])}
        return stats, episodes, [(list(s["ep_true_rets"]), list(s["ep_lens"])) for s in segs], None

    def log_line(stats):
        return ("iter %4d  eps %6d  EpLenMean %7.1f  EpRewMean %8.3f  EpTrueRewMean %8.3f  meankl %.4f  g_loss %.4f  e_loss %.4f  g_acc %.3f  e_acc %.3f  %.1fs"
                % (stats["iteration"], stats["EpThisIter"], stats["EpLenMean"], stats["EpRewMean"], stats["EpTrueRewMean"], stats.get("meankl", float("nan")),
                   stats["generator_loss"], stats["expert_loss"], stats["generator_acc"], stats["expert_acc"], stats["TimeElapsed"]))

    return train_loop.run(pi, iterate, window=40, log_line=log_line, names=locals(), max_iters=max_iters, max_timesteps=max_timesteps,
                          max_seconds=max_seconds, callback=callback, log=log, group=group, log_dir=log_dir, empty_mean=float("nan"),
                          len_mean_iter=False,
                          columns=("optimgain", "meankl", "entloss", "surrgain", "entropy", "ev_tdlam_before") + LOSS_NAMES
                          + ("EpLenMean", "EpRewMean", "EpTrueRewMean", "EpThisIter", "EpisodesSoFar", "TimestepsSoFar", "TimeElapsed")
                          + (train_loop.ERR_KEYS if log_reward_terms else ()))
