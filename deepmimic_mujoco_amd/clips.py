"""`ClipSet`: K mocap clips for ONE batch, every environment imitating one of them (include/dmenv.h dm_mocap_create_set).

DeepMimic trains one policy on a set of motions and picks a motion as an episode starts.  The set is the host-side mirror of what the library
builds on the device: the clips' tables concatenated row-wise, one record per clip {row0, n_frames, dt, loop, shift_x, shift_y, cdf}, and the
float64 cdf of the draw weights whose last entry is exactly 1.0.  `Batch(cm, None, None, n, clips=ClipSet(...))` makes the multi-clip batch.
"""
import numpy as np

from . import _abi as A
from .mocap import MocapDM


def clip_cdf(weights):
    """The draw's cdf as the library computes it: the float64 running sum of the weights over their total, the last entry exactly 1.0."""
    w = [float(x) for x in weights]
    if not w or any(not (x >= 0.0) or x == float("inf") for x in w):
        raise ValueError("clip weights must be finite and >= 0")
    total = 0.0
    for x in w:
        total += x
    if not (total > 0.0) or total == float("inf"):
        raise ValueError("clip weights must have a positive, finite sum")
    cdf, run = [], 0.0
    for x in w:
        run += x
        cdf.append(run / total)
    cdf[-1] = 1.0
    return np.asarray(cdf, dtype=np.float64)


def draw_clip(cdf, u):
    """The clip a draw u in [0, 1) selects: the first c with u < cdf[c] (step_rules.h ClipArgs::episode_clip)."""
    c = 0
    while c < len(cdf) - 1 and not (u < cdf[c]):
        c += 1
    return c


class ClipSet(object):
    def __init__(self, clips, weights=None, imitation_spec=None):
        """clips: clip names / mocap files / loaded `MocapDM` objects, 1..MAX_CLIPS of them.  weights: the probabilities (up to their sum) with which
        clip_mode "episode" draws a clip; None: uniform.  imitation_spec: an imitation.ImitationSpec — every clip then carries its feature table (reward
        modes 3 and 4); the tables' shared parameters (all but 13..15: cycle shift and loop flag) must be equal across the set."""
        clips = list(clips)
        if not 1 <= len(clips) <= A.MAX_CLIPS:
            raise ValueError("a clip set holds 1..%d clips, got %d" % (A.MAX_CLIPS, len(clips)))
        self.names, self.mocaps = [], []
        for c in clips:
            if isinstance(c, MocapDM):
                m, name = c, getattr(c, "name", "clip%d" % len(self.mocaps))
            else:
                m = MocapDM(); m.load_mocap(c); name = str(c)
            self.names.append(name); self.mocaps.append(m)
        K = len(self.mocaps)
        self.weights = np.ones(K) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
        if self.weights.shape != (K,):
            raise ValueError("clip weights: one per clip (%d), got %d" % (K, self.weights.size))
        self.cdf = clip_cdf(self.weights)
        self.n_frames = np.asarray([m.data_config.shape[0] for m in self.mocaps], dtype=np.int32)
        self.row0 = np.concatenate([[0], np.cumsum(self.n_frames)[:-1]]).astype(np.int32)
        self.dt = np.asarray([float(m.dt) for m in self.mocaps], dtype=np.float64)
        self.data_config = np.concatenate([np.asarray(m.data_config, dtype=np.float64) for m in self.mocaps], 0)
        self.data_vel = np.concatenate([np.asarray(m.data_vel, dtype=np.float64) for m in self.mocaps], 0)
        self.imitation = None                  # per clip (table [F,112], params [32])
        self.imit_table = None                 # the concatenation [sum F, 112]
        if imitation_spec is not None:
            self.imitation = [imitation_spec.table_for(m) for m in self.mocaps]
            p0 = np.asarray(self.imitation[0][1], dtype=np.float64)
            shared = np.r_[0:13, 16:32]
            for k, (_t, p) in enumerate(self.imitation):
                if not np.array_equal(np.asarray(p, dtype=np.float64)[shared], p0[shared]):
                    raise ValueError("clip %r: imitation parameters 0..12 and 16..31 must be equal across the set" % (self.names[k],))
            self.imit_table = np.concatenate([np.asarray(t, dtype=np.float64) for t, _p in self.imitation], 0)

    def __len__(self):
        return len(self.mocaps)

    def records(self):
        """one dict per clip: {row0, n_frames, dt, loop, shift_x, shift_y, cdf} — the device's ClipRec (loop and shifts 0 without imitation tables)"""
        out = []
        for k in range(len(self)):
            p = np.zeros(32) if self.imitation is None else np.asarray(self.imitation[k][1], dtype=np.float64)
            out.append(dict(row0=int(self.row0[k]), n_frames=int(self.n_frames[k]), dt=float(self.dt[k]), loop=float(p[15]), shift_x=float(p[13]),
                            shift_y=float(p[14]), cdf=float(self.cdf[k])))
        return out

    def default_assignment(self, n_envs, env_offset=0):
        """clip of env e of a shard starting at global env `env_offset`: (env_offset + e) % K, whatever the sharding"""
        return ((int(env_offset) + np.arange(int(n_envs))) % len(self)).astype(np.int32)

    def episode_clip(self, seed, genv, episode):
        """the clip clip_mode "episode" draws for (seed, global env, episode counter): the device's RNG at stream index 128 against the cdf"""
        return draw_clip(self.cdf, _rng_uniform(seed, genv, episode, 128))


_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _rng_uniform(seed, genv, episode, k):
    """host mirror of the kernels' counter-based RNG (csrc/step_rules.h rng_uniform)"""
    h = _mix64((seed & _M64) ^ _mix64(((genv & 0xFFFFFFFF) * 0x100000001B3 + 0x1234567) & _M64))
    h = _mix64(h ^ ((((episode & 0xFFFFFFFF) << 32) | (k & 0xFFFFFFFF)) & _M64))
    return float(h >> 11) * (1.0 / 9007199254740992.0)
