"""TEST INFRASTRUCTURE: the cases of the external-push tests, shared by the testbench tests (test_push.py) and the device tests (test_gpu_push.py):
the states, the schedules, and the checks that drive any batch with the interface of deepmimic_mujoco_amd.batch.Batch."""
import numpy as np

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.perturb import PushSchedule, ScheduleMirror
from tests import helpers as H
from tests import push_numpy as PN

NBODIES = 13
# wait 0..3 and duration 1..3: at most 6 steps from one push's start to the next's, so every env begins at least 4 pushes within 24 steps
BUSY = dict(bodies=list(range(1, 14)), force=(50.0, 400.0), duration=(1, 3), wait=(0, 3), z=(-0.3, 0.3))
SEED = 1234


def busy_schedule():
    return PushSchedule(**BUSY)


f64r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # the float32-rounded numbers, as float64


def states(n, seed=5, rounded=False):
    """n varied states (helpers.varied_states) with unit root quaternions; rounded: every number rounded to float32 first (what a dtype=32 batch holds)"""
    idx, q, v, ws, _c = H.varied_states(n, seed=seed)
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    return (idx, f64r(q), f64r(v), f64r(ws)) if rounded else (idx, q, v, ws)


def impulses(n, seed=11, rounded=False):
    P = np.random.RandomState(seed).uniform(-30.0, 30.0, size=(n, 3))
    return f64r(P) if rounded else P


def load(batch, idx, q, v, ws):
    batch.set(A.F_QACC_WARMSTART, ws)
    batch.set_state(q, v, frame_idx=idx)


def untouched_fields(batch):
    """everything a push must leave bit for bit"""
    return {f: batch.get(f).copy() for f in (A.F_QPOS, A.F_QACC_WARMSTART, A.F_TIME, A.F_FRAME_IDX, A.F_FRAME_INIT, A.F_CYCLE, A.F_EPISODE)}


def assert_untouched(batch, before):
    for f, val in before.items():
        assert np.array_equal(batch.get(f), val), "field %d changed under a push" % f


_REF = {}


def reference_dqvel(n, bits=64, rounded=False):
    """push_numpy's dqvel for env e of states(n) under impulses(n)[e] on body e % 13 + 1, evaluated in float`bits` with that oracle build's kinematics and
    M; computed once per case and shared (do not modify).  The float32 rule's pair is (bits=32, rounded=True) against (bits=64, rounded=True)."""
    key = (n, bits, rounded)
    if key not in _REF:
        from oracle import oracle as O
        cm = H.compiled_model()
        od = O.Data(O.Model(dtype=bits))
        _idx, q, _v, _ws = states(n, rounded=rounded)
        P = impulses(n, rounded=rounded)
        dt = np.float32 if bits == 32 else np.float64
        out = np.stack([PN.push_dqvel(cm, od, q[e], e % NBODIES + 1, P[e], dt).astype(np.float64) for e in range(n)])
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def run_schedule_against_mirror(batch, n, steps, schedule, seed=SEED, env_offset=0, reset_at=None, reset_mask=None, mirror=None, rng_seed=3):
    """Step `batch` (schedule set by the caller's configuration below) `steps` times and hold DM_F_PUSH_STATE (exactly) and DM_F_PUSH_FORCE (1e-12
    absolute) to the host mirror after EVERY step.  reset_at: a step index before which dm_batch_reset(mode 0, hard) on reset_mask makes the episode counters
    diverge.  -> (the per-step list of (state, force) copies, pushes begun per env, bodies seen per env)"""
    mirror = mirror or ScheduleMirror(schedule, n, seed=seed, env_offset=env_offset)
    rng = np.random.RandomState(rng_seed)
    trace = []
    begun = np.zeros(n, dtype=np.int64); seen = [set() for _ in range(n)]
    for t in range(steps):
        if reset_at is not None and t == reset_at:
            batch.reset(0, 1, reset_mask)
        ep = batch.get(A.F_EPISODE)
        last = mirror.state[:, 4].copy(); last_ep = mirror.state[:, 0].copy()
        mirror.step(ep)
        batch.step(rng.randn(n, A.NU) * 0.3)
        st, F = batch.get(A.F_PUSH_STATE), batch.get(A.F_PUSH_FORCE)
        assert np.array_equal(st, mirror.state), (t, st, mirror.state)
        assert np.abs(F - mirror.force).max() <= 1e-12, (t, np.abs(F - mirror.force).max())
        for e in range(n):
            new = mirror.state[e, 4] - (last[e] if last_ep[e] == mirror.state[e, 0] else 0)
            if new > 0:
                begun[e] += new; seen[e].add(int(mirror.state[e, 3]))
        trace.append((st.copy(), F.copy()))
    return trace, begun, seen
