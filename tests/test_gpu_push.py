"""External pushes on the device (dm_batch_push, dm_batch_set_push_schedule; kernels_push.hip): the scripted push against the numpy restatement and against
momentum, the schedule's launch against the host mirror on every launch form, against its scripted twin bit for bit, and the launch forms that must fall
back to step launches while a schedule is set.  tests/push_cases.py has the cases; tests/test_push.py runs the same kernel source on the wave testbench.

Bars.  Restatement and momentum: the suite's 1e-9 relative.  libdmenv32.so: the float32 rule of tests/float32_cases.py — push_numpy in float32 with the
float32 oracle's kinematics and M against the float64 evaluation of the same float32-rounded inputs gives e32 per env; the kernel stays within MARGIN = 4
of its max and of its median.  Mirror: DM_F_PUSH_STATE exactly, DM_F_PUSH_FORCE to 1e-12.  Everything else: bit for bit."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch
from deepmimic_mujoco_amd.perturb import ScheduleMirror
from deepmimic_mujoco_amd.policy import MlpPolicy
from deepmimic_mujoco_amd.termination import fall_body_mask
from tests import helpers as H
from tests import push_cases as PC
from tests.float32_cases import MARGIN
from tests.gpu_batch import DEV, STATE, assert_bits, horizon_rows, queued_step, stacked, state_of

pytestmark = pytest.mark.gpu
STEPS = 24


def make(n, dtype=64, packed=0, pipeline=1, autoreset=0, max_steps=0, seed=PC.SEED, schedule=None, reward_mode=0, queue=0):
    mc = H.mocap()
    b = Batch(H.compiled_model(), mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt), dtype=dtype)
    b.set_option(A.OPT_SEED, seed); b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_AUTORESET, autoreset); b.set_option(A.OPT_REWARD_MODE, reward_mode)
    if pipeline > 1:
        b.set_option(A.OPT_PIPELINE, pipeline)
    if max_steps:
        b.set_option(A.OPT_MAX_EPISODE_STEPS, max_steps)
    if queue:
        b.set_option(A.OPT_STEP_QUEUE, queue)
    if schedule is not None:
        b.set_push_schedule(schedule)
    return b


def load_states(b, n, rounded=False):
    idx, q, v, ws = PC.states(n, rounded=rounded)
    PC.load(b, idx, q, v, ws)
    return idx, q, v, ws


# ---- dm_batch_push against the restatement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 1])
def test_push_matches_the_restatement(n):
    b = make(n)
    load_states(b, n)
    v0 = b.get(A.F_QVEL).copy(); keep = PC.untouched_fields(b)
    b.push(np.arange(n, dtype=np.int32) % 13 + 1, PC.impulses(n))
    dv = b.get(A.F_QVEL) - v0
    ref = PC.reference_dqvel(n)
    errs = [H.rel_err(dv[e], ref[e]) for e in range(n)]
    print("dm_batch_push against push_numpy, n = %d: max rel err %.3e" % (n, max(errs)))
    assert max(errs) <= 1e-9
    PC.assert_untouched(b, keep)
    b.close()


def test_push_float32_library_within_the_float32_envelope():
    n = 13
    b = make(n, dtype=32)
    load_states(b, n, rounded=True)
    v0 = b.get(A.F_QVEL).copy(); keep = PC.untouched_fields(b)
    b.push(np.arange(n, dtype=np.int32) % 13 + 1, PC.impulses(n, rounded=True))
    dv = b.get(A.F_QVEL) - v0
    ref64, ref32 = PC.reference_dqvel(n, 64, True), PC.reference_dqvel(n, 32, True)
    e32 = np.array([H.rel_err(ref32[e], ref64[e]) for e in range(n)])
    err = np.array([H.rel_err(dv[e], ref64[e]) for e in range(n)])
    print("float32 push: e32 median %.3e max %.3e | kernel median %.3e max %.3e" % (np.median(e32), e32.max(), np.median(err), err.max()))
    assert err.max() <= MARGIN * e32.max() and np.median(err) <= MARGIN * np.median(e32)
    PC.assert_untouched(b, keep)
    b.close()


def test_push_untouched_envs_and_argument_errors():
    n = 4
    b = make(n)
    load_states(b, n)
    v0 = b.get(A.F_QVEL).copy(); keep = PC.untouched_fields(b)
    P = PC.impulses(n)
    b.push([3, 0, 5, 2], np.vstack([np.zeros(3), P[1], P[2], P[3]]), mask=[1, 1, 0, 0])          # zero impulse | body 0 | masked out twice
    assert v0.tobytes() == b.get(A.F_QVEL).tobytes()
    for body, imp in (([3, 0, 5, 14], P), ([3, -1, 5, 2], P), ([1, 1, 1, 1], np.where(np.arange(12).reshape(4, 3) == 7, np.inf, P)),
                      ([1, 1, 1, 1], np.where(np.arange(12).reshape(4, 3) == 2, np.nan, P))):
        with pytest.raises(A.DmenvError):
            b.push(body, imp)
    assert v0.tobytes() == b.get(A.F_QVEL).tobytes()
    # device arrays are not read back: a body out of range or a non-finite impulse leaves its env untouched, the others are pushed
    bad = P.copy(); bad[2, 1] = np.nan
    b.push(torch.tensor([3, 14, 5, 2], dtype=torch.int32, device=DEV), torch.as_tensor(bad, device=DEV))
    b.sync()
    v1 = b.get(A.F_QVEL)
    assert v1[1:3].tobytes() == v0[1:3].tobytes() and np.abs(v1[0] - v0[0]).max() > 1e-3 and np.abs(v1[3] - v0[3]).max() > 1e-3
    PC.assert_untouched(b, keep)
    b.close()


def test_push_changes_the_linear_momentum_by_the_impulse():
    """sum_b m_b dv_b = Rz(-hd) p with v_b from dm_batch_state_features before and after: independent of the restatement"""
    n = 13
    cm = H.compiled_model()
    b = make(n)
    _idx, q, _v, _ws = load_states(b, n)
    P = PC.impulses(n)
    f0 = b.state_features()
    b.push(np.arange(n, dtype=np.int32) % 13 + 1, P)
    f1 = b.state_features()
    vel = lambda f: f[:, 93:].reshape(n, 13, 6)[:, :, :3]
    dp = np.einsum("b,ebk->ek", cm.body_mass[1:14], vel(f1) - vel(f0))
    w, x, y, z = q[:, 3], q[:, 4], q[:, 5], q[:, 6]
    hd = np.arctan2(2 * (x * y + w * z), 1 - 2 * (y * y + z * z))           # the root's x axis in the world: (1 - 2 (y^2 + z^2), 2 (x y + w z), .)
    c, s = np.cos(-hd), np.sin(-hd)
    want = np.stack([c * P[:, 0] - s * P[:, 1], s * P[:, 0] + c * P[:, 1], P[:, 2]], 1)
    err = H.rel_err(dp, want)
    print("momentum change against the impulse: rel err %.3e" % err)
    assert err <= 1e-9
    b.close()


# ---- the schedule against the mirror ---------------------------------------------------------------------------------------------------------------------------
class DeviceSteps(object):
    """a batch stepped with device tensors (what DM_OPT_PIPELINE needs to pipeline), behind the interface run_schedule_against_mirror drives"""

    def __init__(self, b):
        self.b = b
        self.keep = []

    def step(self, action):
        return queued_step(self.b, action, 1, self.keep)

    def __getattr__(self, name):
        return getattr(self.b, name)


@pytest.mark.parametrize("n,packed,pipeline", [(5, 0, 1), (5, 2, 1), (8, 0, 2), (8, 2, 2)], ids=["one-env", "packed-partial-slot", "pipeline-2", "packed-pipeline-2"])
def test_schedule_follows_the_mirror_step_by_step(n, packed, pipeline):
    """auto-reset on and a limit of 7 steps: the termination launch's resets start episodes, whose pushes are drawn afresh"""
    b = make(n, packed=packed, pipeline=pipeline, autoreset=1, max_steps=7, schedule=PC.busy_schedule())
    b.reset(0, 1)
    drv = DeviceSteps(b) if pipeline > 1 else b
    _trace, begun, seen = PC.run_schedule_against_mirror(drv, n, STEPS, PC.busy_schedule())
    assert b.get(A.F_EPISODE).min() >= 1 + STEPS // 7          # dm_batch_reset, then one more episode per 7 steps at least
    assert begun.min() >= 3
    b.close()


# ---- the twin --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed,dtype", [(0, 64), (2, 64), (0, 32)], ids=["one-env", "packed-ext", "one-env-f32"])
def test_scheduled_batch_equals_its_scripted_twin_bit_for_bit(packed, dtype):
    n, cm = 6, H.compiled_model()
    a = make(n, dtype=dtype, packed=packed, autoreset=1, max_steps=7, schedule=PC.busy_schedule())
    b = make(n, dtype=dtype, packed=packed, autoreset=1, max_steps=7)
    for x in (a, b):
        x.reset(0, 1)
    mirror = ScheduleMirror(PC.busy_schedule(), n, seed=PC.SEED)
    rng = np.random.RandomState(9)
    pushes = 0
    for t in range(STEPS):
        body, _F = mirror.step(a.get(A.F_EPISODE))
        act = rng.randn(n, A.NU) * 0.3
        oa = a.step(act)
        b.push(body, a.get(A.F_PUSH_FORCE) * (cm.timestep * 1.0))
        ob = b.step(act)
        pushes += int((body > 0).sum())
        for x, y in zip(oa, ob):
            assert x.tobytes() == y.tobytes(), t
        assert_bits(state_of(a), state_of(b), t)
    assert pushes >= 3 * n
    a.close(); b.close()


# ---- rollout, step queue and step_act fall back to step launches -----------------------------------------------------------------------------------------------
def reference_loop(n, acts, **cfg):
    """dm_batch_step with host arrays, step after step -> (obs, rew, done stacked, the final state and push records)"""
    b = make(n, schedule=PC.busy_schedule(), **cfg)
    b.reset(0, 1)
    outs = [tuple(x.copy() for x in b.step(acts[t])) for t in range(len(acts))]
    res = {"rows%d" % k: np.stack([o[k] for o in outs]) for k in range(3)}
    res.update(state_of(b, STATE + (A.F_PUSH_STATE, A.F_PUSH_FORCE)))
    b.close()
    return res


@pytest.mark.parametrize("horizon_term", [0, 1])
def test_rollout_and_step_queue_with_a_schedule_are_step_launches(horizon_term):
    n, T = 6, 12
    cfg = dict(packed=1, autoreset=1, max_steps=7)
    acts = np.random.RandomState(4).randn(T + 1, n, A.NU) * 0.3
    ref = reference_loop(n, acts[:T], **cfg)
    assert ref[A.F_PUSH_STATE][:, 4].min() >= 1 and ref[A.F_EPISODE].min() >= 2
    # dm_batch_rollout
    b = make(n, schedule=PC.busy_schedule(), queue=8, **cfg)
    b.set_option(106, 1)                                       # one launch per horizon wherever the batch allows it: a schedule does not
    b.set_option(A.OPT_HORIZON_TERMINATION, horizon_term)
    b.reset(0, 1)
    ac, *out = horizon_rows(T, n, act=acts)[:4]
    b.rollout(ac, out, 1)
    b.sync()
    got = {"rows%d" % k: out[k].cpu().numpy() for k in range(3)}
    got.update(state_of(b, STATE + (A.F_PUSH_STATE, A.F_PUSH_FORCE)))
    assert_bits(ref, got, "rollout")
    assert b.queue_stats() == (0, 0, 0)
    b.close()
    # DM_OPT_STEP_QUEUE
    b = make(n, schedule=PC.busy_schedule(), queue=8, **cfg)
    b.set_option(106, 1); b.set_option(A.OPT_HORIZON_TERMINATION, horizon_term)
    b.reset(0, 1)
    drv = DeviceSteps(b)
    for t in range(T):
        drv.step(acts[t])
        assert b.queue_stats() == (0, 0, 0)
    b.join(); b.sync()
    got = stacked(b, drv.keep, STATE + (A.F_PUSH_STATE, A.F_PUSH_FORCE), actions=False)
    assert_bits(ref, got, "step queue")
    b.close()


@pytest.mark.parametrize("packed", [0, 1])
def test_step_act_with_a_schedule_equals_the_step_loop(packed):
    n, T = 6, 12
    cfg = dict(packed=packed, autoreset=1)
    pol = MlpPolicy(device=DEV, seed=2)
    W = pol.pack()
    b = make(n, schedule=PC.busy_schedule(), **cfg)
    b.reset(0, 1)
    ac, *out, vp = horizon_rows(T, n, a0=np.random.RandomState(4).randn(n, A.NU) * 0.3)
    for t in range(T):
        b.step_act(ac[t], 1, (out[0][t], out[1][t], out[2][t]), W, ac[t + 1], vp[t], True, 11, t)
    b.sync()
    got = {"rows%d" % k: out[k].cpu().numpy() for k in range(3)}
    got.update(state_of(b, STATE + (A.F_PUSH_STATE, A.F_PUSH_FORCE)))
    acts = ac.cpu().numpy()
    b.close()
    assert np.abs(acts[1:]).max() > 0                           # the policy wrote the later actions
    ref = reference_loop(n, acts[:T], **cfg)
    assert ref[A.F_PUSH_STATE][:, 4].min() >= 1
    assert_bits(ref, got, "step_act")


# ---- off after on ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_schedule_turned_on_and_off_again_leaves_no_trace():
    n = 6
    acts = np.random.RandomState(4).randn(8, n, A.NU) * 0.3
    res = []
    for touched in (False, True):
        b = make(n, packed=1, autoreset=1)
        if touched:
            b.set_push_schedule(PC.busy_schedule()); b.set_push_schedule(None)
        b.reset(0, 1)
        outs = [tuple(x.copy() for x in b.step(a)) for a in acts]
        r = {"rows%d" % k: np.stack([o[k] for o in outs]) for k in range(3)}
        r.update(state_of(b, STATE + (A.F_PUSH_STATE, A.F_PUSH_FORCE)))
        res.append(r)
        b.close()
    assert_bits(res[0], res[1])
    assert (res[1][A.F_PUSH_STATE] == np.array([-1, 0, 0, 0, 0])).all() and not res[1][A.F_PUSH_FORCE].any()
