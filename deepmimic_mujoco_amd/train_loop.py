"""The loop of the reference's `learn()` functions (src/trpo.py:214-319, src/gail.py:245-364, ppo1's pposgd_simple), written once for
trpo.learn, ppo.learn and gail.learn: stopping rules, world / rank, the two log files of rank 0, the all-reduced episode counts, the episode
windows, the counters, the history.  What an iteration DOES is the caller's `iterate`.  Host-side plumbing; no device code."""
import os
import time
from collections import deque

import torch


def segments(pi, env, horizon, fused=None, bootstrap_time_limit=False, reward_terms=False):
    """-> (segment generator, this rank's env count) over a DPVecEnv, or a list of them (pipelined rollouts).  bootstrap_time_limit: the segments carry
    "vboot", the critic's value of the states a time limit cut off (rollout.SegmentCollector).  reward_terms: they carry `err_sums` (reward_terms_stat)."""
    from .rollout import can_fuse, pipelined_segment_generator, traj_segment_generator
    if isinstance(env, (list, tuple)):          # several env batches of this rank, stepped concurrently on their own streams
        return pipelined_segment_generator(pi, list(env), horizon, stochastic=True, bootstrap_time_limit=bootstrap_time_limit,
                                           reward_terms=reward_terms), sum(e.num_envs for e in env)
    # fused (default when possible): the policy step runs inside the env step kernel, one launch per rollout step
    use_fused = can_fuse(pi, env) if fused is None else bool(fused)
    return traj_segment_generator(pi, env, horizon, stochastic=True, fused=use_fused, bootstrap_time_limit=bootstrap_time_limit, reward_terms=reward_terms), env.num_envs


# learn(log_reward_terms=True): the imitation reward's five errors (imitation.TERM_NAMES) of the states each segment ends in, logged after the learner's own keys
ERR_KEYS = ("ErrPose", "ErrVel", "ErrEndEff", "ErrRoot", "ErrCom")


def reward_terms_stat(stats, seg, group=None):
    """ErrPose .. ErrCom: the mean over the environments (of every rank) whose last step of `seg` was not done of the imitation reward's five errors at
    the state the segment ends in (a segment of segments(reward_terms=True); nothing is added otherwise).  One small copy to the host per segment."""
    sums = getattr(seg, "err_sums", None)
    if sums is None:
        return
    import torch.distributed as dist
    from .trpo import _world
    if _world(group) > 1:
        sums = sums.clone()
        dist.all_reduce(sums, group=group)
    v = sums.tolist()
    for k, x in zip(ERR_KEYS, v[:5]):
        stats[k] = x / max(1.0, v[5])


def truncation_stat(stats, seg):
    """TruncThisIter: the episodes the time limit alone truncated in `seg` (a bootstrap_time_limit segment; nothing is added otherwise)."""
    count = getattr(seg, "trunc_count", None)
    n = count() if count is not None else None
    if n is not None:
        stats["TruncThisIter"] = n


def run(pi, iterate, *, window, columns, log_line, names, max_iters=0, max_timesteps=0, max_seconds=0, callback=None, log=print, group=None,
        log_dir=None, empty_mean=0.0, len_mean_iter=True):
    """Iterate until `max_iters` iterations, `max_timesteps` (global) or `max_seconds` have passed; -> the list of per-iteration stat dicts.

    iterate(timesteps_so_far) -> (stats, episodes, monitor, advance):
        stats     the iteration's own numbers; the loop adds the episode statistics and the counters to it
        episodes  {statistic: values of the episodes this iteration counts}, "EpLenMean" (their lengths) first: each statistic is the mean
                  over the last `window` values (`empty_mean` before the first episode); the lengths also give EpThisIter and, with
                  `len_mean_iter`, EpLenMeanIter
        monitor   [(returns, lengths), ...] of this rank's episodes for the monitor file
        advance   what TimestepsSoFar grows by; None: by the counted episodes' lengths (src/gail.py:361)
    columns: progress.csv's, in order.  log_line(stats) -> the line rank 0 logs.  names: what `callback(locals, globals)` finds in its first
    dict beside iters_so_far, timesteps_so_far, episodes_so_far and history (the caller's `locals()`: learner, pi, ...).
    With `log_dir`, rank 0 writes progress.csv (logger CSV, src/logger.py:101-135) and monitor.json.monitor.csv (bench.Monitor) there."""
    import torch.distributed as dist
    from .trpo import _world
    world = _world(group)
    rank = dist.get_rank(group) if world > 1 else 0
    episodes_so_far = timesteps_so_far = iters_so_far = 0
    tstart = time.time()
    buffers = {}
    history = []
    progress = monitor = None
    if log_dir and rank == 0:
        from .logio import ProgressCsv, MonitorWriter
        os.makedirs(log_dir, exist_ok=True)
        progress = ProgressCsv(os.path.join(log_dir, "progress.csv"))
        monitor = MonitorWriter(os.path.join(log_dir, "monitor.json"), t_start=tstart)
    try:
        while True:
            if callback:
                callback(dict(names, iters_so_far=iters_so_far, timesteps_so_far=timesteps_so_far, episodes_so_far=episodes_so_far,
                              history=history), globals())
            if max_timesteps and timesteps_so_far >= max_timesteps:
                break
            if max_iters and iters_so_far >= max_iters:
                break
            if max_seconds:
                # the deadline is a per-process wall clock: decide collectively (MAX over ranks), or a rank that breaks first leaves
                # the others waiting forever in the next update's all-reduces
                stop = time.time() - tstart >= max_seconds
                if world > 1:
                    flag = torch.tensor([1.0 if stop else 0.0], dtype=torch.float32, device=pi.device)
                    dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=group)
                    stop = bool(flag.item() > 0)
                if stop:
                    break
            stats, episodes, monitor_rows, advance = iterate(timesteps_so_far)
            lens = list(episodes["EpLenMean"])
            # a device tensor in one process too: EpLenMeanIter is its quotient, and on a GPU torch divides by a host number by multiplying with
            # its reciprocal, which is not always the host's quotient in the last bit (logged values stay what they were)
            sums = torch.tensor([len(lens), sum(lens)], dtype=torch.float64, device=pi.device)
            if world > 1:                                        # :300-302 allgather of (ep_lens, ep_rets): the sums suffice here
                dist.all_reduce(sums, group=group)
            n_eps, n_steps = int(sums[0]), int(sums[1])
            for k, v in episodes.items():
                buffers.setdefault(k, deque(maxlen=window)).extend(v)
            episodes_so_far += n_eps
            timesteps_so_far += n_steps if advance is None else advance
            iters_so_far += 1
            stats.update({k: float(sum(b) / len(b)) if len(b) else empty_mean for k, b in buffers.items()})
            if len_mean_iter:
                stats["EpLenMeanIter"] = float(sums[1] / max(1.0, float(sums[0])))
            stats.update(EpThisIter=n_eps, EpisodesSoFar=episodes_so_far, TimestepsSoFar=timesteps_so_far, TimeElapsed=time.time() - tstart,
                         iteration=iters_so_far)
            history.append(stats)
            if progress is not None:
                progress.writekvs({k: stats.get(k) for k in columns})
                for rets, ep_lens in monitor_rows:
                    monitor.write_episodes(rets, ep_lens)
            if log and rank == 0:
                log(log_line(stats))
    finally:
        if progress is not None:
            progress.close(); monitor.close()
    return history
