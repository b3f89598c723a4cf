"""Multi-GPU sharding of the environment index range and the per-horizon rollout exchange.

Environments are independent, so the only collective is the one the learner needs: every `horizon` steps each rank
contributes its [T, N_local, 87] float32 block (obs 56 | action 28 | reward | done | vpred) to an all-gather
(RCCL over xGMI when the backend is "nccl"; "gloo" in the CPU tests).  Env e of the global range lives on rank
e // N_local, and per-env RNG streams are keyed by the GLOBAL env id, so results do not depend on the sharding.
"""
ROW = 87  # 56 obs + 28 act + reward + done + vpred


def shard_range(n_global, rank, world):
    """Contiguous block [lo, hi) of the global env range owned by `rank` (sizes differ by at most one)."""
    base, rem = divmod(int(n_global), int(world))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class RolloutBlock(object):
    """Accumulates T steps of (obs, action, reward, done[, vpred]) for the local shard; all-gathers on demand."""

    def __init__(self, horizon, n_local, device="cpu"):
        import torch
        self.T, self.n = int(horizon), int(n_local)
        self.buf = torch.zeros((self.T, self.n, ROW), dtype=torch.float32, device=device)
        self.t = 0

    def append(self, obs, action, reward, done, vpred=None):
        row = self.buf[self.t]
        if obs.shape[-1] != 56:
            raise ValueError("the rollout block's row is 87 wide (56 obs | 28 act | reward | done | vpred): observations of width %d (obs_mode "
                             "'deepmimic') are not gathered" % obs.shape[-1])
        row[:, :56] = obs; row[:, 56:84] = action; row[:, 84] = reward; row[:, 85] = done
        if vpred is not None:
            row[:, 86] = vpred
        self.t += 1
        return self.t == self.T

    def gather(self, out=None):
        """All ranks receive every rank's block: returns [world, T, n_local, 87].  Resets the fill counter."""
        import torch
        import torch.distributed as dist
        self.t = 0
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return self.buf.unsqueeze(0)
        world = dist.get_world_size()
        if out is None:
            out = torch.empty((world,) + tuple(self.buf.shape), dtype=self.buf.dtype, device=self.buf.device)
        dist.all_gather_into_tensor(out.view(world * self.T, self.n, ROW), self.buf)
        return out


class DoubleBufferedGather:
    """Per-horizon all-gather of the rollout block, overlapped with stepping: two [T, n, 87] blocks per rank; while block k
    travels (async all-gather on the collective's own stream) the envs fill block 1 - k.  `row(t)` returns the row to fill at
    step t (first making sure that this block's previous gather has finished), `commit(t)` launches the gather when step t
    completes a horizon, `drain()` waits for everything outstanding.  Single-process runs degenerate to one local block.

    Backend "nccl" (RCCL) gathers device tensors in place.  Backend "gloo" has no device all-gather: a block on a GPU is first
    copied to pinned host memory (stream-ordered), the gather runs between host buffers (async, gloo's own threads) and the
    result stays on the host in `gathered_host[k]` — the path the world-2 tests and single-GPU multi-rank runs use."""

    def __init__(self, horizon, n_local, device="cpu", world=None, collective=None, ob_width=56):
        """ob_width: the width of the observations the caller will write into the rows; the 87-wide row holds 56 (obs_mode "dp_env_v3") and nothing else.
        collective: run the multi-rank code path (two blocks, the all-gather into `gathered`) — default: when the process group has more
        than one rank; True forces it for a group of ONE rank, which executes the same RCCL calls where only one GPU is visible."""
        import torch
        import torch.distributed as dist
        if world is None:
            world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        if int(ob_width) != 56:
            raise ValueError("the gathered rollout row is 87 wide (56 obs | 28 act | reward | done | vpred): observations of width %d (obs_mode "
                             "'deepmimic') are not gathered" % int(ob_width))
        self.T, self.n, self.world = int(horizon), int(n_local), int(world)
        self.collective = (self.world > 1) if collective is None else bool(collective)
        nb = 2 if self.collective else 1
        self.blocks = [torch.zeros((self.T, self.n, ROW), dtype=torch.float32, device=device) for _ in range(nb)]
        on_gpu = torch.device(device).type == "cuda"
        self.host_staged = self.collective and on_gpu and dist.get_backend() == "gloo"
        self.gathered = self.gathered_host = self.host_blocks = None
        if self.collective and self.host_staged:
            self.host_blocks = [torch.zeros((self.T, self.n, ROW), dtype=torch.float32).pin_memory() for _ in range(nb)]
            self.gathered_host = [torch.empty((self.world * self.T, self.n, ROW), dtype=torch.float32) for _ in range(nb)]
        elif self.collective:
            self.gathered = [torch.empty((self.world * self.T, self.n, ROW), dtype=torch.float32, device=device) for _ in range(nb)]
        self.pending = [None] * nb
        self.completed = 0                      # gathers launched so far

    def _k(self, t):
        return (t // self.T) % len(self.blocks)

    def row(self, t):
        k = self._k(t)
        if t % self.T == 0 and self.pending[k] is not None:
            self.pending[k].wait(); self.pending[k] = None
        return self.blocks[k][t % self.T]

    def block(self, t):
        """The whole [T, n, 87] block step t belongs to (for producers that fill a block in one go at the end of a horizon)."""
        k = self._k(t)
        if self.pending[k] is not None:
            self.pending[k].wait(); self.pending[k] = None
        return self.blocks[k]

    def commit(self, t):
        """Call after step t's row has been written.  Returns the index of the gathered buffer when a gather was launched."""
        if self.collective and (t + 1) % self.T == 0:
            import torch
            import torch.distributed as dist
            k = self._k(t)
            if self.host_staged:
                self.host_blocks[k].copy_(self.blocks[k], non_blocking=True)
                torch.cuda.current_stream(self.blocks[k].device).synchronize()      # the host copy is complete before gloo reads it
                self.pending[k] = dist.all_gather_into_tensor(self.gathered_host[k], self.host_blocks[k], async_op=True)
            else:
                self.pending[k] = dist.all_gather_into_tensor(self.gathered[k], self.blocks[k], async_op=True)
            self.completed += 1
            return k
        return None

    def result(self, k):
        """The gathered [world * T, n, 87] buffer of slot k (device tensor, or the host tensor on the host-staged path)."""
        return self.gathered_host[k] if self.host_staged else self.gathered[k]

    def drain(self):
        for k in range(len(self.pending)):
            if self.pending[k] is not None:
                self.pending[k].wait(); self.pending[k] = None
