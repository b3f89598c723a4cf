"""Device-resident rollouts: the batched form of the reference's `traj_segment_generator` and what it is made of.

`SegmentCollector` is one env batch's side of the generator: `launch()` enqueues a horizon of policy and env steps, `collect()` turns the filled
buffers into a `Segment`.  Its optional features are objects that own their state: `EpisodeScan` (the returns and lengths of the episodes that end in
a segment; a second one for the env's own reward beside a reward giver's), `_TimeLimitBootstrap` (the critic's value of the states a time limit cut
off) and `HorizonKernelChoice` (four environments per wavefront or one for the next horizon launch).  `traj_segment_generator` and
`pipelined_segment_generator` drive one collector or several; `add_vtarg_and_adv` (GAE) and `flatten_segment` are what the learners apply to a segment.
`env_obs_width` is the one place that knows how wide an env's observation is.  The multi-GPU exchange of rollout blocks lives in exchange.py; its names
are re-exported here.
"""
from .batch import batch_option
from .exchange import ROW, DoubleBufferedGather, RolloutBlock, shard_range  # noqa: F401


def add_vtarg_and_adv(seg, gamma, lam):
    """GAE(lambda) of `src/trpo.py:83-94` for N environments at once.

    seg["rew"], seg["vpred"], seg["new"] are [T, N]; seg["nextvpred"] is [N].  Per env column this is the reference's
    reversed loop verbatim:  nonterminal = 1 - new[t+1];  delta = rew[t] + gamma * vpred[t+1] * nonterminal - vpred[t];
    adv[t] = delta + gamma * lam * nonterminal * adv[t+1];  tdlamret = adv + vpred  — float32 like the reference's
    `np.empty(T, 'float32')`.  T sequential steps of N-wide vector ops on the tensors' device (no host round trip).

    With seg["vboot"] [T, N] (SegmentCollector(bootstrap_time_limit=True)): vboot[t] is the value of the state step t left where a time limit
    truncated the episode there, 0 elsewhere, and delta[t] gains gamma * vboot[t] — the truncated state is worth the critic's value, not 0;
    the chain still cuts at new[t+1].  Without the key nothing changes."""
    import torch
    rew, vpred, new = seg["rew"], seg["vpred"], seg["new"]
    T = rew.shape[0]
    vboot = seg["vboot"] if "vboot" in seg else None
    if (rew.is_cuda and rew.dim() == 2 and rew.dtype == torch.float32 and vpred.dtype == torch.float32 and new.dtype == torch.int32
            and rew.is_contiguous() and vpred.is_contiguous() and new.is_contiguous()):
        # one launch of the k_gae kernel (csrc/policy_kernel.h) instead of T small ones; k_gae_boot with bootstrap values
        from . import _abi as A
        L, p = A.load(), A.ptr
        nxt = seg["nextvpred"].to(torch.float32).contiguous()
        adv = torch.empty_like(rew); ret = torch.empty_like(rew)
        if vboot is None:
            A.check(L.dm_gae(p(rew), p(vpred), p(new), p(nxt), p(adv), p(ret), T, rew.shape[1], float(gamma), float(lam),
                             A.stream(rew.device)), L)
        else:
            vb = vboot.to(device=rew.device, dtype=torch.float32).contiguous()
            if tuple(vb.shape) != tuple(rew.shape):
                raise ValueError("seg['vboot'] must have the shape of seg['rew']")
            A.check(L.dm_gae_boot(p(rew), p(vpred), p(new), p(nxt), p(vb), p(adv), p(ret), T, rew.shape[1], float(gamma), float(lam),
                                  A.stream(rew.device)), L)
        seg["adv"], seg["tdlamret"] = adv, ret
        return seg
    new1 = torch.cat([new.to(torch.float32), torch.zeros_like(new[:1], dtype=torch.float32)], 0)     # np.append(new, 0)
    vp1 = torch.cat([vpred.to(torch.float32), seg["nextvpred"].to(torch.float32)[None]], 0)          # np.append(vpred, nextvpred)
    nonterminal = 1.0 - new1[1:]
    if vboot is None:
        delta = rew.to(torch.float32) + gamma * vp1[1:] * nonterminal - vp1[:-1]
    else:
        delta = rew.to(torch.float32) + gamma * (vp1[1:] * nonterminal + vboot.to(torch.float32)) - vp1[:-1]
    decay = (gamma * lam) * nonterminal
    adv = torch.empty_like(delta)
    last = torch.zeros_like(delta[0])
    for t in range(T - 1, -1, -1):
        last = delta[t] + decay[t] * last
        adv[t] = last
    seg["adv"] = adv
    seg["tdlamret"] = adv + vpred.to(torch.float32)
    return seg


def can_fuse(pi, env, device=None):
    """True when `SegmentCollector(fused=True)` is possible: the policy step can run inside the env step kernel (dm_batch_step_act)."""
    import torch
    device = torch.device(pi.device if device is None else device)
    return (device.type == "cuda" and getattr(pi, "native", False) and hasattr(getattr(env, "batch", None), "step_act")
            and getattr(env.batch, "can_step_act", True) and getattr(env, "obs_mode", "dp_env_v3") == "dp_env_v3" and getattr(pi, "ob_dim", 0) == 56 and getattr(pi, "ac_dim", 0) == 28 and getattr(pi, "hid_size", 0) == 100)


def env_obs_width(env):
    """Width of the observation `env` hands to a policy: the step launch's 56 numbers in obs_mode "dp_env_v3" (and for an env object that names no mode),
    else what its observation space says (171 for "deepmimic")."""
    if getattr(env, "obs_mode", "dp_env_v3") == "dp_env_v3":
        return 56
    return int(env.observation_space.shape[0])


def _pack_is_stale(pi):
    """the fused launches read the policy's packed float32 block: True when `pi.pack()` has to run first"""
    return getattr(pi, "_dirty", False) or getattr(pi, "_packed", None) is None


class _PendingEpisodes:
    """Episode statistics of a segment whose records are still on their way to the host (EpisodeScan.native)."""

    def __init__(self, scan, event):
        self.scan, self.event, self.out = scan, event, None

    def result(self):
        if self.out is None:
            import numpy as np
            _cnt, rec, h_cnt, h_rec = self.scan.records
            self.event.synchronize()
            k = min(int(h_cnt[0]), rec.shape[0])
            r = h_rec[:min(k, h_rec.shape[0])].numpy()
            if k > h_rec.shape[0]:
                r = np.concatenate([r, rec[h_rec.shape[0]:k].cpu().numpy()], 0)
            order = np.argsort(r[:, 0], kind="stable")                     # word 0 = t << 32 | env: time-major, then env
            self.out = (r[order, 1].copy().view(np.float64).tolist(), r[order, 2].tolist())
            if self.scan.pending is self:
                self.scan.pending = None
        return self.out


class EpisodeScan(object):
    """One episode stream over consecutive [T, n] segments: return and length of every episode that ends inside a segment, in time-major order (the order in
    which a single-env loop would have appended them, src/trpo.py:72-76), and the carry of the episodes still open at its end."""

    EP_HEAD = 16384                      # episode records fetched with the count in one asynchronous copy (more than that: a second copy)

    def __init__(self, T, n, device):
        import torch
        self.T, self.n, self.device = int(T), int(n), torch.device(device)
        self.cur_ret = torch.zeros(self.n, dtype=torch.float64, device=self.device)     # running return / length of the open episodes
        self.cur_len = torch.zeros(self.n, dtype=torch.int64, device=self.device)
        self.step_idx = torch.arange(1, self.T + 1, device=self.device, dtype=torch.int64)[:, None]
        self.records = None              # native form: (count [1] i32, records [T n, 3] i64) on the device, and their pinned host copies
        self.pending = None              # ... and its one result whose records may still be travelling into them
        if self.device.type == "cuda":
            cap = self.T * self.n
            head = min(cap, self.EP_HEAD)
            self.records = (torch.zeros(1, dtype=torch.int32, device=self.device), torch.empty((cap, 3), dtype=torch.int64, device=self.device),
                            torch.zeros(1, dtype=torch.int32).pin_memory(), torch.empty((head, 3), dtype=torch.int64).pin_memory())

    def scan(self, rew64, done8):
        """-> a `_PendingEpisodes` (device buffers the kernel can walk) or the finished (ep_rets, ep_lens)"""
        import torch
        if self.device.type == "cuda" and rew64.dtype == torch.float64 and rew64.is_contiguous() and done8.is_contiguous():
            return self.native(rew64, done8)
        return self.torch(rew64, done8.to(torch.bool))

    def native(self, rew64, done8):
        """One launch (dm_episode_scan: thread = env walks its column of the segment) and a host sort of the few episodes that ended, instead
        of ~100 launch-bound tensor ops.  Returns are float64 sums in step order, like the reference's `cur_ep_ret += rew`.  Nothing waits
        here: the records travel to pinned memory behind the kernel, and `_PendingEpisodes.result()` sorts them when somebody asks — the
        learner does while the device is busy with the update's first kernels."""
        import torch
        from . import _abi as A
        dev = self.device
        if self.pending is not None:
            self.pending.result()                                          # (its pinned buffers are about to be overwritten)
        cnt, rec, h_cnt, h_rec = self.records
        L, p = A.load(), A.ptr
        A.check(L.dm_episode_scan(p(rew64), p(done8), self.T, self.n, p(self.cur_ret), p(self.cur_len), p(cnt), rec.shape[0], p(rec),
                                  A.stream(dev)), L)
        h_cnt.copy_(cnt, non_blocking=True)
        h_rec.copy_(rec[:h_rec.shape[0]], non_blocking=True)
        ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(dev))
        self.pending = _PendingEpisodes(self, ev)
        return self.pending

    def torch(self, rew64, done):
        """the same in [T, n]-wide tensor ops on any device; done: bool [T, n].  -> (ep_rets, ep_lens)"""
        import torch
        T, n, device = self.T, self.n, self.device
        cur_ret, cur_len = self.cur_ret, self.cur_len
        csum = torch.cumsum(rew64, 0)
        ends = done.nonzero()                                              # [K, 2] (t, env), sorted by t then env
        ep_rets, ep_lens = [], []
        if ends.numel():
            te, ee = ends[:, 0], ends[:, 1]
            # previous end of the same env inside the segment (or -1): sort by (env, t) and shift
            order = torch.argsort(ee * T + te)
            te_s, ee_s = te[order], ee[order]
            prev_t = torch.full_like(te_s, -1)
            same = ee_s[1:] == ee_s[:-1]
            prev_t[1:] = torch.where(same, te_s[:-1], torch.full_like(te_s[:-1], -1))
            seg_ret = csum[te_s, ee_s] - torch.where(prev_t >= 0, csum[prev_t.clamp(min=0), ee_s], torch.zeros_like(csum[te_s, ee_s]))
            seg_len = te_s - prev_t
            opening = prev_t < 0                                           # first end of that env: add what it carried in
            seg_ret = seg_ret + torch.where(opening, cur_ret[ee_s], torch.zeros_like(seg_ret))
            seg_len = seg_len + torch.where(opening, cur_len[ee_s], torch.zeros_like(seg_len))
            inv = torch.empty_like(order); inv[order] = torch.arange(order.numel(), device=device)
            ep_rets = seg_ret[inv].tolist(); ep_lens = seg_len[inv].tolist()
        # carry the open episodes into the next segment
        last_end = torch.where(done, self.step_idx.expand(T, n), torch.zeros((T, n), dtype=torch.int64, device=device)).amax(0)   # 1-based
        tail_ret = csum[-1] - torch.where(last_end > 0, csum[(last_end - 1).clamp(min=0), torch.arange(n, device=device)], torch.zeros_like(csum[-1]))
        self.cur_ret = torch.where(last_end > 0, tail_ret, cur_ret + tail_ret)
        self.cur_len = torch.where(last_end > 0, T - last_end, cur_len + T)
        return ep_rets, ep_lens


class Segment(dict):
    """The generator's segment dict.  "ep_rets" / "ep_lens" materialise on first access when the collector left them pending
    (`finish_episode_stats()` does it explicitly — the learner calls it where the host would otherwise wait for the device)."""

    pending_episodes = None
    pending_true = None                  # with a reward_giver: the env's own returns ("ep_true_rets"), also on their way to the host
    info = None                          # how the segment was produced (launch form, overflow rate of the packed path): diagnostics, not data
    pending_trunc = None                 # bootstrap_time_limit: (pinned int32 [1], event) — the truncation log's count on its way to the host
    err_sums = None                      # reward_terms: float64 [6] on the device — the imitation reward's five errors summed over the envs whose last step
                                         # of the segment was not done, then their number (train_loop.reward_terms_stat takes the mean)
    _trunc = None

    def trunc_count(self):
        """Episodes the time limit alone truncated inside the segment (the truncation log's count); None without bootstrap_time_limit."""
        if self.pending_trunc is not None:
            h, ev = self.pending_trunc
            if ev is not None:
                ev.synchronize()
            self._trunc = int(h[0])
            self.pending_trunc = None
        return self._trunc

    def finish_episode_stats(self):
        self.trunc_count()
        if self.pending_episodes is not None:
            rets, lens = self.pending_episodes.result()
            self.pending_episodes = None
            dict.__setitem__(self, "ep_rets", rets); dict.__setitem__(self, "ep_lens", lens)
        if self.pending_true is not None:
            rets, _ = self.pending_true.result()
            self.pending_true = None
            dict.__setitem__(self, "ep_true_rets", rets)

    def _pending(self, key):
        return ((key in ("ep_rets", "ep_lens") and self.pending_episodes is not None)
                or (key == "ep_true_rets" and self.pending_true is not None))

    def __missing__(self, key):
        if self._pending(key):
            self.finish_episode_stats()
            return dict.__getitem__(self, key)
        raise KeyError(key)

    def __contains__(self, key):
        return dict.__contains__(self, key) or self._pending(key)

    # whoever walks the dict sees all of it
    def __iter__(self):
        self.finish_episode_stats(); return dict.__iter__(self)

    def __len__(self):
        self.finish_episode_stats(); return dict.__len__(self)

    def keys(self):
        self.finish_episode_stats(); return dict.keys(self)

    def items(self):
        self.finish_episode_stats(); return dict.items(self)

    def values(self):
        self.finish_episode_stats(); return dict.values(self)

    def get(self, key, default=None):
        return self[key] if key in self else default


class _TimeLimitBootstrap(object):
    """SegmentCollector(bootstrap_time_limit=True): the env's truncation log sized to the segment, and the buffers its records are read into.  An
    environment is truncated at most once per M steps, and a segment's first truncation may fall on any of its rows: at most T // M + 1 per environment,
    so a log of n (T // M + 1) records never overflows."""

    def __init__(self, pi, env, T, n, device, as_buf):
        import torch
        from . import _abi as A
        self.pi, self.env, self.T, self.n, self.device, self.as_buf = pi, env, T, n, device, as_buf
        M = int(env.max_episode_steps or 0)
        if M <= 0:
            raise ValueError("bootstrap_time_limit needs an env with a time limit (DPVecEnv(max_episode_steps=M), M > 0)")
        # a multi-clip batch with the 171-wide observation: the phase of a truncated state runs over the length of the clip the env was on, which a log
        # record does not carry.  With clip_mode "fixed" it is still the env's clip when the log is read; with "episode" it has been redrawn by then.
        self.many_clips = getattr(env, "clip_set", None) is not None and len(env.clip_set) > 1
        if self.many_clips and env_obs_width(env) != 56 and getattr(env, "clip_mode", "fixed") != "fixed":
            raise ValueError("bootstrap_time_limit with obs_mode=\"deepmimic\" on a list of motions needs clip_mode=\"fixed\": the truncation log does not record the "
                             "clip a truncated state was on, and clip_mode=\"episode\" has redrawn it when the log is read")
        C = self.capacity = n * (T // M + 1)
        env.batch.set_option(A.OPT_TRUNCATION_LOG, C)
        self.log = (torch.zeros(1, dtype=torch.int32, device=device), torch.zeros((C, 4), dtype=torch.int32, device=device),
                    torch.zeros((C, A.NQ), dtype=torch.float64, device=device), torch.zeros((C, A.NV), dtype=torch.float64, device=device))
        self.ob = torch.zeros((C, env_obs_width(env)), dtype=torch.float64, device=device)
        self.slot = torch.arange(C, device=device, dtype=torch.int64)
        self.vboot = torch.zeros((T, n), dtype=torch.float32, device=device)
        self.h_count = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(2)] if device.type == "cuda" else None
        self.h_k = 0

    def clear(self):
        """the log's count and tick start again (stream-ordered, nothing is copied but the old count)"""
        self.env.batch.truncations(clear=True, out=(self.as_buf(self.log[0]), None, None, None))

    def values(self, seg):
        """seg["vboot"] [T, n] f32: the critic's value of every state the time limit cut off in this segment, at (tick, env); 0 elsewhere.  All C slots
        of the log become observations and are evaluated (at most n rows for T <= M); the slots at or above the count are masked on the device, so
        nothing waits for the count."""
        import torch
        from . import _abi as A
        from .state_features import phase_of
        b, T, n, as_buf = self.env.batch, self.T, self.n, self.as_buf
        cnt, idx, qp, qv = self.log
        b.truncations(clear=False, out=tuple(as_buf(x) for x in self.log))
        if self.ob.shape[1] == 56:
            torch.cat([qp[:, 7:], qv[:, 6:]], 1, out=self.ob)
        else:
            # the phase the features launch would have given this state had the episode gone on: from the cursors as the step left them
            mode = batch_option(b, A.OPT_REWARD_MODE)
            if self.many_clips:      # (clip_mode "fixed": the record's env is still on the clip it was truncated on; slots beyond the count are masked below)
                lens = torch.tensor([int(x) for x in self.env.clip_set.n_frames], device=idx.device, dtype=torch.int64)
                clip = torch.as_tensor(self.env.clip_ids(), device=idx.device).to(torch.int64)
                F = lens[clip[idx[:, 0].to(torch.int64).clamp(0, n - 1)]]
                k = idx[:, 2].to(torch.int64) + (idx[:, 3].to(torch.int64) if mode in (2, 4) else 0)      # state_features.phase_of with a length per record
                phase = ((k % F).to(torch.float64) / F.to(torch.float64)).contiguous()
            else:
                phase = phase_of(mode, idx[:, 2], idx[:, 3], b.n_frames).contiguous()
            b.state_features(as_buf(self.ob), qpos=as_buf(qp), qvel=as_buf(qv), phase=as_buf(phase))
        with torch.no_grad():
            v = self.pi.forward_value(self.ob).to(torch.float32)
        tick, e = idx[:, 1].to(torch.int64), idx[:, 0].to(torch.int64)
        ok = (self.slot < cnt.to(torch.int64)) & (tick >= 0) & (tick < T) & (e >= 0) & (e < n)
        flat = torch.where(ok, tick * n + e, torch.zeros_like(tick))
        # (tick, env) is unique among the valid records, the others add 0 to row 0: the sum IS the scatter, whatever order the records arrived in
        self.vboot.zero_()
        self.vboot.view(-1).index_add_(0, flat, torch.where(ok, v, torch.zeros_like(v)))
        seg["vboot"] = self.vboot.clone()
        if self.h_count is not None:
            h = self.h_count[self.h_k]; self.h_k ^= 1
            h.copy_(cnt, non_blocking=True)
            ev = torch.cuda.Event(); ev.record(torch.cuda.current_stream(self.device))
            seg.pending_trunc = (h, ev)
        else:
            seg.pending_trunc = (cnt.clone(), None)


class HorizonKernelChoice(object):
    """Four environments per wavefront or one, for the next horizon (envs that leave the choice open: DPVecEnv.horizon_packed_ok).
    The horizon launch re-steps an environment beyond the packed path's capacities inside its wave, which holds up its three
    partners: fine at the 1e-4 rates of a falling / walking population, not for one that stands on both feet (32+ rows) most of the
    time.  Decided from the last horizon's own statistics (redo rate on the packed path, largest row count on the one-env path):
    a deterministic function of the trajectory."""

    # horizon launch -> one-env steps: an in-wave re-step holds a wave (four environments) for about one lone one-env step.  Measured on a
    # population learning to stand (tools/train_trpo.py, 4 096 envs x 128 steps, MI355X; profiles/r04_ab_kernel_variants.md): 38 / 42 / 46 /
    # 52 / 55 / 58-60 ms per horizon at 0.2 / 0.8 / 1.3 / 2.6 / 3.7 / 5 % of env-steps re-stepped (the rate levels off near 5 %) against
    # 67 ms for the same population through one-env launches — the packed horizon stays ahead to about 7 %.  (Round 3's 2 % came from a cost
    # estimate; a run that crossed it at 2.02 % lost a quarter of its rollout throughput for the rest of the training.)
    REDO_RATE_MAX = 7e-2
    HEAVY_ROWS = 38                        # the way back to the packed horizon launch: nobody above this (it holds _abi.PACKED_MAXROWS = 40 rows per env)

    def __init__(self, env, T, n):
        import os
        self.env, self.T, self.n = env, int(T), int(n)
        if os.environ.get("DM_HORIZON_REDO_RATE_MAX"):                   # (experiments: tools/prof_train.sh)
            self.REDO_RATE_MAX = float(os.environ["DM_HORIZON_REDO_RATE_MAX"])
        self.packed_now = None                     # what choose() picked for the last horizon (None: none yet)
        self.kernel_switches = 0
        self.last_redo_rate = None
        self._redo_seen = None                     # the batch's redo counter after the last choice (None: no horizon yet)

    def choose(self):
        """Set the batch to the kernel for the next horizon.  -> the callable that undoes it after the horizon's calls, or None for an env whose
        configuration pins the kernel (nothing is touched then)."""
        from . import _abi as A
        b = self.env.batch
        if not self.env.horizon_packed_ok:
            return None
        # the choice holds for the collector's rollout calls only: what the batch was set to (and its per-step chooser, if on) comes back
        # after each call, so `DPVecEnv.step` callers of the same env are not moved to a kernel that is the slower one per step
        was_mode = batch_option(b, A.OPT_PACKED)        # (0 one env per wave, 1 packed, 2 packed with the three-set code per step)
        was_on = bool(was_mode)
        on = was_on if self.packed_now is None else self.packed_now
        if self._redo_seen is None:                                         # first horizon: start packed
            want = True
        elif on:
            self.last_redo_rate = (b.redo_total() - self._redo_seen) / float(self.T * self.n)
            want = self.last_redo_rate <= self.REDO_RATE_MAX
        else:
            want = int(b.get(A.F_NEFC).max()) <= self.HEAVY_ROWS
        if want != on:
            self.kernel_switches += 1
        self.packed_now = want
        was_auto = b.suspend_auto()                                         # (suspended, not reset: its counters go on afterwards)
        if want != was_on:
            b.set_option(A.OPT_PACKED, 1 if want else 0)
        self._redo_seen = b.redo_total()

        def restore():
            if want != was_on:
                b.set_option(A.OPT_PACKED, was_mode)
            if was_auto:
                b.resume_auto()                                             # (rebaselined: the horizon's in-wave re-steps are not the per-step chooser's evidence)
        return restore


class SegmentCollector(object):
    """One env batch's side of `traj_segment_generator`, split into `launch()` (enqueue T policy + env steps, no host wait) and
    `collect()` (episode bookkeeping, the one host transfer per segment) so that several env batches can be in flight at once.
    With `stream` (a torch CUDA stream) everything this collector enqueues runs on that stream.

    With `reward_giver` (gail.TransitionClassifier: src/gail.py:27's generator) the segment's rewards are D's: one `reward_into` call
    (dm_disc_reward, one launch) per segment after the horizon fills a second [T, N] float64 buffer from the segment's (ob, ac) — D is
    fixed for the whole segment, so this is the reference's per-step `reward_giver.get_reward(ob, ac)` (:78).  seg["rew"] and
    "ep_rets" then come from it, "ep_true_rets" from the env's reward through a second episode scan with its own carry (:85-91)."""

    def __init__(self, pi, env, horizon, stochastic=True, device=None, first_reset="rsi", stream=None, fused=False, reward_giver=None,
                 bootstrap_time_limit=False, reward_terms=False):
        """reward_terms (an env with reward="imitation"): one dm_batch_imitation_terms call per segment, on the states the segment ends in, behind the
        horizon's launches — the segment then carries `err_sums` (Segment); nothing is added to a step."""
        import torch
        from . import _abi as A
        self.pi, self.env, self.T, self.stochastic, self.stream = pi, env, int(horizon), stochastic, stream
        n, T = env.num_envs, self.T
        self.n = n
        device = torch.device(pi.device if device is None else device)
        self.device = device
        self.as_buf = (lambda x: x) if device.type == "cuda" else (lambda x: x.numpy())   # host tensors: shared-memory views
        self.terms = None                          # reward_terms: the [n, 28] rows of the states the segment ended in
        if reward_terms:
            if batch_option(env.batch, A.OPT_REWARD_MODE) != 3:
                raise ValueError("reward_terms needs an env with reward=\"imitation\" (the batch's cursors name the compared frame in that mode only)")
            self.terms = torch.zeros((n, A.NTERMS), dtype=torch.float64, device=device)
        self.bootstrap = _TimeLimitBootstrap(pi, env, T, n, device, self.as_buf) if bootstrap_time_limit else None
        f32, f64 = torch.float32, torch.float64
        self.ob_width = env_obs_width(env)
        self.ob64 = torch.zeros((T + 1, n, self.ob_width), dtype=f64, device=device)   # row t: observation the policy sees at step t
        # obs_mode "deepmimic": the step launch writes its 56 numbers here, then dm_batch_state_features fills the segment's row from the state it left
        self.ob56 = torch.zeros((n, 56), dtype=f64, device=device) if self.ob_width != 56 else None
        self.ac64 = torch.zeros((T + 1, n, 28), dtype=f64, device=device)         # row T: the action already drawn for ob64[T] (fused path)
        self.rew64 = torch.zeros((T, n), dtype=f64, device=device)
        self.done8 = torch.zeros((T, n), dtype=torch.uint8, device=device)
        self.vpreds = torch.zeros((T + 1, n), dtype=f32, device=device)
        self.first = torch.ones(n, dtype=torch.int32, device=device)               # `new` of row 0: carried over from the last segment
        self.last_ac = torch.zeros((n, 28), dtype=f32, device=device)              # prevac of row 0 (trpo.py:29 samples a random one)
        self.episodes = EpisodeScan(T, n, device)                                  # of the segment's reward
        self.reward_giver = reward_giver
        if reward_giver is not None:                                               # (these two exist only then)
            self.drew64 = torch.zeros((T, n), dtype=f64, device=device)            # D's reward of every (ob, ac) of the segment
            self.true_episodes = EpisodeScan(T, n, device)                         # of the env's own reward
        # fused path: the env step kernel also runs the policy on the observation it produced (dm_batch_step_act), one launch per step.
        # As in the reference's generator (src/trpo.py:47-56) the action for the first observation of a segment was then drawn BEFORE the
        # update in between (by the policy that finished the last segment) and only its value is re-evaluated afterwards.
        if fused and not can_fuse(pi, env, device):
            raise ValueError("fused rollout steps need the native policy kernel (56-100-100-28) and a device-resident env batch")
        self.fused = bool(fused)
        self.have_ac0 = False
        self.kernel_choice = HorizonKernelChoice(env, T, n)
        with self._on_stream():
            env.reset(first_reset, out=self.as_buf(self.ob64[0]))                  # trpo.py:32 `ob = env.reset()` (RSI); later episodes: noisy init

    # what the last horizon ran on (None: no choice made yet) and how often the choice changed: read by the benchmark and tools/rollout_policy_bench.py
    _packed_now = property(lambda self: self.kernel_choice.packed_now)
    kernel_switches = property(lambda self: self.kernel_choice.kernel_switches)

    def _on_stream(self):
        import contextlib
        import torch
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _follow_current_stream(self):
        """with `stream`: what the caller's stream has enqueued so far (parameter updates, the last collect's copies) comes before what the side stream gets next"""
        if self.stream is not None:
            import torch
            self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def launch(self):
        import torch
        self._follow_current_stream()                                               # parameters / filter updated by the learner are visible
        if self.fused and _pack_is_stale(self.pi):
            self.pi.pack()                                                          # (on the caller's stream, before the side stream forks)
            self._follow_current_stream()
        with self._on_stream(), torch.no_grad():                                    # (the learner may hold the parameters with requires_grad)
            if self.bootstrap is not None:
                self.bootstrap.clear()                                              # tick 0 = this segment's first step
            if not self.fused:
                self._launch_steps()
            elif hasattr(self.env.batch, "rollout"):
                self._launch_fused_horizon()
            else:
                self._launch_fused_steps()

    def _launch_steps(self):
        """T policy forwards and T env step launches; the value of the observation after the segment (:49-52) behind them.  The action for that
        observation is sampled at the top of the next segment, i.e. from the policy as updated in between."""
        pi, batch, as_buf, fs = self.pi, self.env.batch, self.as_buf, getattr(self.env, "frame_skip", 1)
        ob64, ac64, rew64, done8, vpreds = self.ob64, self.ac64, self.rew64, self.done8, self.vpreds
        for t in range(self.T):
            pi.act(self.stochastic, ob64[t], out=ac64[t], vpred_out=vpreds[t])                           # :49
            if self.ob56 is None:
                batch.step(as_buf(ac64[t]), fs, (as_buf(ob64[t + 1]), as_buf(rew64[t]), as_buf(done8[t])))   # :66, one launch
            else:
                batch.step(as_buf(ac64[t]), fs, (as_buf(self.ob56), as_buf(rew64[t]), as_buf(done8[t])))
                batch.state_features(as_buf(ob64[t + 1]))
        vpreds[self.T] = pi.forward(ob64[self.T])[1]

    def _first_fused_action(self):
        if not self.have_ac0:
            self.pi.act(self.stochastic, self.ob64[0], out=self.ac64[0], vpred_out=self.vpreds[0])      # very first step: :49
        else:
            self.vpreds[0] = self.pi.forward_value(self.ob64[0])                                         # :56, the updated policy's value

    def _launch_fused_horizon(self):
        """the whole horizon in one call (dm_batch_rollout): on the packed path ONE launch in which every wavefront runs its four
        environments through all T steps at its own pace; on the one-env path T step launches issued without returning here"""
        pi, env, T = self.pi, self.env, self.T
        self._first_fused_action()
        restore = self.kernel_choice.choose() if getattr(env, "horizon_packed_ok", False) else None
        try:
            env.batch.rollout(self.ac64, (self.ob64[1:], self.rew64, self.done8), getattr(env, "frame_skip", 1), pi._packed, self.vpreds[1:],
                              self.stochastic, pi._seed, pi._counter + 1)
            pi._counter += T
            env.batch.join()
        finally:                                        # (also when the rollout raises: the batch must not be left on the collector's kernel choice)
            if restore is not None:
                restore()                               # per-step callers of the same env keep the kernel THEY were given

    def _launch_fused_steps(self):
        pi, batch, fs = self.pi, self.env.batch, getattr(self.env, "frame_skip", 1)
        ob64, ac64, rew64, done8, vpreds = self.ob64, self.ac64, self.rew64, self.done8, self.vpreds
        self._first_fused_action()
        for t in range(self.T):                                                                          # :49 + :66, one launch
            pi._counter += 1
            batch.step_act(ac64[t], fs, (ob64[t + 1], rew64[t], done8[t]), pi._packed, ac64[t + 1], vpreds[t + 1],
                           self.stochastic, pi._seed, pi._counter)
        batch.join()

    def _reward_term_sums(self, seg):
        """reward_terms: behind the horizon's launches, before the next segment's — the states the segment ends in"""
        import torch
        self.env.batch.imitation_terms(out=self.as_buf(self.terms))
        keep = (self.done8[-1] == 0).to(torch.float64)          # an env the last step reset shows its fresh episode's row: left out
        seg.err_sums = torch.cat([(self.terms[:, :5] * keep[:, None]).sum(0), keep.sum()[None]])

    def _scan_episodes(self, seg, rew64, true64):
        """episode statistics: pending on the segment where the scan kernel runs, else finished lists under its keys"""
        eps = self.episodes.scan(rew64, self.done8)
        true = self.true_episodes.scan(true64, self.done8) if true64 is not None else None
        if isinstance(eps, _PendingEpisodes):
            seg.pending_episodes, seg.pending_true = eps, true
        else:
            seg["ep_rets"], seg["ep_lens"] = eps
            if true is not None:
                seg["ep_true_rets"] = true[0]

    def collect(self):
        import os
        import time
        import torch
        T, device = self.T, self.device
        f32 = torch.float32
        seg = Segment()
        with self._on_stream():                        # (on the stream the batch is on: reading its log there needs no change of stream)
            if self.bootstrap is not None:
                self.bootstrap.values(seg)
            if self.terms is not None:
                self._reward_term_sums(seg)
        if self.stream is not None:
            torch.cuda.current_stream(device).wait_stream(self.stream)
        prof = os.environ.get("DM_TRPO_PROFILE") and device.type == "cuda"
        if prof:
            torch.cuda.synchronize(device); t_c = time.perf_counter()
        ob64, ac64, rew64, done8, vpreds = self.ob64, self.ac64, self.rew64, self.done8, self.vpreds
        true64 = None
        if self.reward_giver is not None:
            with torch.no_grad():
                self.reward_giver.reward_into(ob64[:T], ac64[:T], self.drew64)        # gail.py:78, the whole segment at once
            true64, rew64 = rew64, self.drew64
        if device.type == "cuda":
            done8.to(torch.bool)                       # (read by nothing since the scans take done8: the launch stays where it was, dropping it is a change of its own)
        new = torch.cat([self.first[None], done8[:-1].to(torch.int32)], 0)
        acs = ac64[:T].to(f32)
        prevacs = torch.cat([self.last_ac[None], acs[:-1]], 0)
        seg.info = {"packed": self._packed_now, "kernel_switches": self.kernel_switches, "redo_rate": self.kernel_choice.last_redo_rate}
        self._scan_episodes(seg, rew64, true64)
        seg.update({"ob": ob64[:T].to(f32), "rew": rew64.to(f32), "vpred": vpreds[:T].clone(), "new": new, "ac": acs, "prevac": prevacs,
                    "nextvpred": vpreds[T] * (1 - done8[-1].to(f32))})
        # the carry into the next segment
        self.first = done8[-1].to(torch.int32)
        self.last_ac = acs[-1].clone()
        ob64[0].copy_(ob64[T])
        if self.fused:
            ac64[0].copy_(ac64[T]); self.have_ac0 = True
        self._follow_current_stream()                  # the copies above are ordered before the next launch
        if prof:
            torch.cuda.synchronize(device); self.collect_ms = (time.perf_counter() - t_c) * 1e3
            seg["collect_ms"] = self.collect_ms
        return seg


def traj_segment_generator(pi, env, horizon, stochastic=True, device=None, first_reset="rsi", fused=False, reward_giver=None, bootstrap_time_limit=False,
                           reward_terms=False):
    """Batched `traj_segment_generator` (src/trpo.py:27-80): N envs advance in lock step on the device.

    pi: policy.MlpPolicy; env: DPVecEnv created with autoreset="init" — the kernel then applies, on `done`, exactly what
    the reference does on the host (`env.reset(); ob = env.env.reset_model_init()`, :77-79) and returns the fresh
    episode's observation.  Yields, every `horizon` steps, the reference's segment dict with a leading [T, N] shape:
    ob [T,N,56] f32, ac / prevac [T,N,28] f32, rew / vpred [T,N] f32, new [T,N] int32 (new[t] = ob[t] starts an episode),
    nextvpred [N], ep_rets / ep_lens (lists of finished episodes, host numbers — the only host transfer, once per segment).

    Per step the loop issues only the policy forward and ONE env launch: the policy writes its action and value straight
    into row t of the segment buffers, and `dm_batch_step` reads that action row and writes the next observation, the
    reward and the done flag straight into rows t+1 / t / t of theirs (float64, as the C ABI produces them).  With `fused=True`
    (see `can_fuse`) even the policy forward is gone: the env step kernel runs it on the observation it has just produced
    (`dm_batch_step_act`), a step is ONE launch, and with `DM_OPT_PIPELINE` on the batch consecutive steps overlap.  The float32
    segment views, `new`, `prevac` and the episode statistics are derived once per segment with [T, N]-wide ops.
    Nothing leaves the device or the stream.

    reward_giver (src/gail.py:27-92): the rewards are the discriminator's (see SegmentCollector); the segment also carries
    "ep_true_rets", the env's returns of the same episodes.

    bootstrap_time_limit (env with max_episode_steps > 0): the segment also carries "vboot" [T,N] f32, the critic's value of every state the time
    limit cut off (_TimeLimitBootstrap.values), which `add_vtarg_and_adv` adds to the one-step target there.

    reward_terms (env with reward="imitation"): the segment also carries `err_sums` (Segment), from one terms launch per segment."""
    c = SegmentCollector(pi, env, horizon, stochastic, device, first_reset, fused=fused, reward_giver=reward_giver, bootstrap_time_limit=bootstrap_time_limit,
                         reward_terms=reward_terms)
    while True:
        c.launch()
        yield c.collect()


def pipelined_segment_generator(pi, envs, horizon, stochastic=True, first_reset="rsi", fused=False, bootstrap_time_limit=False, reward_terms=False):
    """The same segments from SEVERAL env batches (e.g. two halves of a GPU's envs) stepped concurrently, each on its own CUDA
    stream: the whole T-step chain of every batch (policy forward -> env step -> policy forward ...) is enqueued without a host
    wait, so while one batch's env kernel drains its last, cheap workgroups the other batch's policy / env kernels fill the freed
    wave slots — the overlap `DM_OPT_PIPELINE` gives open-loop stepping, for the closed loop.  Yields one segment dict whose env
    axis is the concatenation of the batches (episode lists concatenated in batch order)."""
    import torch
    cols = [SegmentCollector(pi, e, horizon, stochastic, None, first_reset, stream=torch.cuda.Stream(device=pi.device), fused=fused,
                             bootstrap_time_limit=bootstrap_time_limit, reward_terms=reward_terms) for e in envs]
    while True:
        if _pack_is_stale(pi):
            pi.pack()                                  # once, on the current stream, before the side streams fork from it
        for c in cols:
            c.launch()
        segs = [c.collect() for c in cols]
        for sg in segs:
            sg.finish_episode_stats()                  # (the lists are concatenated below)
        out = Segment()
        if bootstrap_time_limit:
            out._trunc = sum(sg.trunc_count() for sg in segs)
        if reward_terms:
            out.err_sums = sum(sg.err_sums for sg in segs)
        for k in segs[0]:                              # ("vboot", when there, is [T, N] like "rew": it joins along the env axis)
            if k in ("ep_rets", "ep_lens"):
                out[k] = [x for sg in segs for x in sg[k]]
            elif k == "nextvpred":
                out[k] = torch.cat([sg[k] for sg in segs], 0)
            else:
                out[k] = torch.cat([sg[k] for sg in segs], 1)
        yield out


def flatten_segment(seg):
    """[T, N, ...] -> [T*N, ...] views env-major (each env's T steps contiguous), the layout the reference's learner
    consumes when several workers' segments are concatenated."""
    out = {}
    for k in ("ob", "ac", "prevac", "rew", "vpred", "new", "adv", "tdlamret"):
        if k in seg:
            v = seg[k]
            out[k] = v.transpose(0, 1).reshape((-1,) + tuple(v.shape[2:]))
    return out
