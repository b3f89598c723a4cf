"""External pushes (include/dmenv.h dm_batch_push / dm_batch_set_push_schedule): DeepMimic's perturbations — a random force on a
random body part for a fraction of a second, which the policy has to recover from (upstream's Perturb / PerturbManager, code.md:949-952).

`PushSchedule` describes the random schedule (which bodies, how long between pushes, how long and how hard each push) and checks it; `ScheduleMirror` is
the float64 host restatement of the rule the device's k_push follows, a state machine over steps, for tests and for callers that want to know ahead of
time what the device will do.  Nothing here pushes anything: the impulse is a HIP kernel (Batch.push, Batch.set_push_schedule)."""
import math

import numpy as np

from . import _abi as A
from .clips import _rng_uniform
from .termination import fall_body_mask


class PushSchedule(object):
    """bodies: a set name of termination.FALL_BODY_SETS, body names and / or model body ids (1..13), or the bit mask itself (termination.fall_body_mask);
    wait, duration: (min, max) env steps between pushes and that a force is held; force: (min, max) newtons; z: (min, max) of the direction's vertical
    component ((0, 0): horizontal).  A single number stands for (x, x).  ValueError outside the ranges of include/dmenv.h dm_push_desc."""

    def __init__(self, bodies, force, duration=(1, 1), wait=(0, 0), z=(0.0, 0.0)):
        self.bodies = fall_body_mask(bodies)
        if self.bodies == 0:
            raise ValueError("a push schedule needs at least one body (pass perturb=None for no pushes)")
        pair = lambda v: (v, v) if np.isscalar(v) else tuple(v)
        self.wait = tuple(int(x) for x in pair(wait))
        self.duration = tuple(int(x) for x in pair(duration))
        self.force = tuple(float(x) for x in pair(force))
        self.z = tuple(float(x) for x in pair(z))
        for name, v in (("wait", self.wait), ("duration", self.duration), ("force", self.force), ("z", self.z)):
            if len(v) != 2:
                raise ValueError("%s = (min, max)" % name)
        if not 0 <= self.wait[0] <= self.wait[1]:
            raise ValueError("wait: 0 <= min <= max env steps")
        if not 1 <= self.duration[0] <= self.duration[1]:
            raise ValueError("duration: 1 <= min <= max env steps")
        if not (all(math.isfinite(x) for x in self.force) and 0.0 <= self.force[0] <= self.force[1]):
            raise ValueError("force: 0 <= min <= max newtons, finite")
        if not -1.0 <= self.z[0] <= self.z[1] <= 1.0:
            raise ValueError("z: -1 <= min <= max <= 1")

    @classmethod
    def coerce(cls, x):
        """None | PushSchedule | dict of the constructor's arguments | the --perturb string -> PushSchedule or None"""
        if x is None or isinstance(x, cls):
            return x
        if isinstance(x, str):
            return cls.parse(x)
        return cls(**dict(x))

    @classmethod
    def parse(cls, text):
        """"bodies=root+chest,force=50:200,duration=2:6,wait=30:90[,z=-0.2:0.2]" (bodies: a set name, or names / ids joined by '+'); "" / "none": None"""
        if text is None or text.strip() in ("", "none"):
            return None
        kw = {}
        for item in text.split(","):
            if "=" not in item:
                raise ValueError("--perturb: expected key=value, got %r" % item)
            k, v = (s.strip() for s in item.split("=", 1))
            if k == "bodies":
                parts = [int(p) if p.isdigit() else p for p in v.split("+")]
                kw[k] = parts[0] if len(parts) == 1 and isinstance(parts[0], str) else parts
            elif k in ("force", "z", "duration", "wait"):
                lo, _, hi = v.partition(":")
                conv = float if k in ("force", "z") else int
                kw[k] = (conv(lo), conv(hi if hi else lo))
            else:
                raise ValueError("--perturb: unknown key %r (bodies, force, duration, wait, z)" % k)
        if "bodies" not in kw or "force" not in kw:
            raise ValueError("--perturb needs bodies= and force=")
        return cls(**kw)

    def desc(self):
        """the ctypes dm_push_desc"""
        return A.PushDesc(self.bodies, self.wait[0], self.wait[1], self.duration[0], self.duration[1], self.force[0], self.force[1], self.z[0], self.z[1])

    def body_list(self):
        return [b for b in range(1, A.NBODY) if (self.bodies >> b) & 1]

    def __repr__(self):
        return "PushSchedule(bodies=%#x, force=%r, duration=%r, wait=%r, z=%r)" % (self.bodies, self.force, self.duration, self.wait, self.z)


def _draw_int(u, lo, hi):
    return lo + min(int(math.floor(u * (hi - lo + 1))), hi - lo)


class ScheduleMirror(object):
    """The schedule's rule in float64 on the host, for n environments: `state` int32 [n,5] {episode_seen, wait, left, body, count} and `force` [n,3] are what
    DM_F_PUSH_STATE and DM_F_PUSH_FORCE read after the same calls.  step(episode) takes DM_F_EPISODE as it stands BEFORE the device's step call and returns
    (body [n] int32, force [n,3]): the push applied ahead of that step (body 0: none); the impulse is force * timestep * n_substeps."""

    def __init__(self, schedule, n_envs, seed=0, env_offset=0):
        self.s = schedule
        self.n = int(n_envs)
        self.seed, self.env_offset = int(seed), int(env_offset)
        self.state = np.zeros((self.n, 5), dtype=np.int32)
        self.state[:, 0] = -1
        self.force = np.zeros((self.n, 3))

    def _u(self, e, ep, j, k):
        return _rng_uniform(self.seed, self.env_offset + e, ep, 256 + 8 * j + k)

    def step(self, episode):
        s, bodies = self.s, self.s.body_list()
        body = np.zeros(self.n, dtype=np.int32)
        force = np.zeros((self.n, 3))
        for e in range(self.n):
            ep = int(episode[e])
            st = self.state[e]
            if st[0] != ep:
                st[0] = ep; st[4] = 0; st[2] = 0
                st[1] = _draw_int(self._u(e, ep, 0, 0), *s.wait)
            if st[2] == 0:
                if st[1] > 0:
                    st[1] -= 1
                    continue
                j = int(st[4])
                st[2] = _draw_int(self._u(e, ep, j, 1), *s.duration)
                st[3] = bodies[min(int(math.floor(self._u(e, ep, j, 2) * len(bodies))), len(bodies) - 1)]
                mag = s.force[0] + self._u(e, ep, j, 3) * (s.force[1] - s.force[0])
                phi = 6.283185307179586476925 * self._u(e, ep, j, 4)
                z = s.z[0] + self._u(e, ep, j, 5) * (s.z[1] - s.z[0])
                rxy = math.sqrt(1.0 - z * z)
                self.force[e] = (mag * (rxy * math.cos(phi)), mag * (rxy * math.sin(phi)), mag * z)
                st[4] += 1
            body[e] = st[3]; force[e] = self.force[e]
            st[2] -= 1
            if st[2] == 0:
                st[1] = _draw_int(self._u(e, ep, int(st[4]), 0), *s.wait)
        return body, force
