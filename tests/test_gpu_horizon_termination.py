"""Early termination inside the horizon launch and the step queue (DM_OPT_HORIZON_TERMINATION; csrc/kernels_rollout_term.hip) on the GPU.

The reference is always the same build's own path with the option OFF — step launches, each followed by the termination launch — on the same batch
configuration, and the comparison is bit for bit: every output row, the state fields, the counters, the reasons, the truncation records.

The per-step kernel of both twins is, for bit identity, the packed one with the three-set code (DPVecEnv(packed=2), DM_OPT_PACKED = 2: 40 constraint rows per environment).
A horizon's waves call that instantiation for an environment near the two-set capacity, so an environment at 33 .. 40 rows — the sunk frames among the
states here sit there — stays on the packed path in both forms.  With the lean per-step kernel (packed=True) the step launches hand such an environment
to the one-env code, whose sums differ from the packed path's in the last bits whether or not termination is on: measured on an MI355X with
packed=True, n = 6, no auto-reset, "alive": done rows equal, 290 of 2 352 observation values differ, by at most 1.1e-14.
The rollout, step-queue and truncation-log comparisons therefore run a second time with packed=True — the configuration the training tools use — where done rows,
reasons, counters, cursors, episodes, the records' ticks and environments and the queue statistics are asserted equal and float rows and state within LEAN_TOL.

Input condition.  The horizon kernel's fall test runs on the four-per-wavefront kinematics, the termination launch's on the one-env kinematics; the
two differ in the last bits, so a decision whose geom lies within HC.BOUNDARY (1e-9 m; float32: the 1e-4 m band of tests/test_gpu_termination.py) of the
rule's boundary is not defined between them.  Every comparison with a fall set first shows, from the states the reference's own steps leave (a probe
batch without termination stepped from the reference's state, step by step), that the inputs hold no such pair."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
from deepmimic_mujoco_amd import termination as TM
from deepmimic_mujoco_amd.rollout import SegmentCollector
from tests import floor_numpy as FN
from tests import helpers as H
from tests import horizon_term_cases as HC
from tests import gpu_batch as GB
from tests.gpu_batch import DEV, assert_bits, assert_bits_or_close, horizon_rows, queued_steps, result, stacked, start, truncation_log

pytestmark = pytest.mark.gpu
SEED = 5
LIMIT = 3
STEPS = 7
DEEPMIMIC = TM.fall_body_mask("deepmimic")
STATE = GB.STATE + GB.TERM_FIELDS


def make(n, on, fall="deepmimic", limit=LIMIT, autoreset="rsi", reward="alive", dtype=64, step_queue=0, log=0, packed=2):
    env = DPVecEnv(n, motion="walk", reward=reward, autoreset=autoreset, seed=SEED, dtype=dtype, packed=packed, step_queue=step_queue,
                   fall_contact_bodies=fall, max_episode_steps=limit, truncation_log=log, horizon_termination=on)
    assert env.packed and env.batch.options.get(A.OPT_HORIZON_TERMINATION, 0) == (1 if on else 0)
    return env


# packed=True (DM_OPT_PACKED 1, the lean per-step kernel): an env-step at 33 .. 40 rows is the one-env code's in the step launches and the packed three-set code's in
# the horizon, two orders of the same float64 sums.  Everything discrete must still be equal; float rows and state may differ by reordered rounding: one env-step is
# some 1e4 float64 operations per value on numbers of order 1 (1e4 x 1.1e-16 = 1e-12 if every rounding error lined up; 1.1e-14 was measured), carried over the
# 7 steps of a horizon whose episodes are cut at 3.  Relative to max(1, |value|).
LEAN_TOL = 1e-12


def assert_same(got, ref, packed=2):
    """packed == 2: bit for bit.  packed is True: integer arrays (done rows, reasons, counters, cursors, episodes) bit for bit, float arrays within LEAN_TOL"""
    assert_bits(got, ref) if packed == 2 else assert_bits_or_close(got, ref, LEAN_TOL)


def check_inputs(n, act, idx, q, v, done_rows, dtype=64, want_mix=True, **cfg):
    """the input condition, and the mix of endings in the horizon: a fall, a time-limit end, a step-own done, episodes that go on"""
    cm = H.compiled_model()
    cfg = dict(cfg, dtype=dtype)
    pre_q, stepdone = GB.states_before_termination(lambda: make(n, False, **cfg), lambda: make(n, False, **dict(cfg, fall=None, limit=0)), idx, q, v, act, 1)
    closest = HC.closest_decision(cm, pre_q, ~stepdone, TM.geoms_of_bodies(DEEPMIMIC, cm.geom_bodyid))      # (the geoms that decide: the fall set's)
    touch = (FN.floor_masks(cm, pre_q.reshape(-1, 35)).reshape(stepdone.shape) & TM.geoms_of_bodies(DEEPMIMIC, cm.geom_bodyid)) != 0
    fall = touch & ~stepdone
    ended = (done_rows != 0) & ~stepdone
    print("closest fall decision %.3e m from its boundary; %d ended by the step, %d fell, %d ended by the limit alone, %d env-steps went on"
          % (closest, stepdone.sum(), fall.sum(), (ended & ~fall).sum(), (done_rows == 0).sum()))
    assert closest > (HC.BOUNDARY if dtype == 64 else HC.BOUNDARY32)
    np.testing.assert_array_equal(ended & fall, fall)                      # every fall ended its episode
    if want_mix:
        assert stepdone.any() and fall.any() and (ended & ~fall).any() and (done_rows == 0).any()


# ---- the option --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_option_values(dtype):
    env = DPVecEnv(4, dtype=dtype, max_episode_steps=3)
    b = env.batch
    for v in (1, 0, 1, 0):
        b.set_option(A.OPT_HORIZON_TERMINATION, v)
    for bad in (2, -1):
        with pytest.raises(A.DmenvError):
            b.set_option(A.OPT_HORIZON_TERMINATION, bad)
    assert b.options[A.OPT_HORIZON_TERMINATION] == 0
    env.close()


# ---- dm_batch_rollout without a policy -------------------------------------------------------------------------------------------------------------
CASES = ([(n, ar, rw, 64, pk) for pk in (2, True) for n in (6, 66) for ar in (None, "rsi", "init") for rw in ("alive", "imitation")]
         + [(66, "rsi", "imitation", 32, 2)])


@pytest.mark.parametrize("n,autoreset,reward,dtype,packed", CASES)
def test_rollout_equals_step_launches(n, autoreset, reward, dtype, packed):
    idx, q, v = HC.states(n, many=n == 66, seed=HC.STATE_SEED if dtype == 64 else HC.STATE_SEED32)
    act = HC.actions(STEPS, n)
    cfg = dict(autoreset=autoreset, reward=reward, dtype=dtype, packed=packed)
    res = []
    for on in (False, True):
        env = make(n, on, **cfg)
        b = env.batch
        assert b.options[A.OPT_PACKED] == (2 if packed == 2 else 1)
        start(b, idx, q, v)
        redo0 = b.redo_total()
        bufs = horizon_rows(STEPS, n, act=act)
        b.rollout(bufs[0], bufs[1:4], 1)
        res.append(result(b, bufs[:4], STATE))
        if on and n == 66:
            assert b.redo_total() - redo0 >= 1                            # the many-row environments were re-stepped inside their waves
        env.close()
    check_inputs(n, act, idx, q, v, res[0]["rows3"], **cfg)
    assert_same(res[1], res[0], packed)


# ---- dm_batch_rollout with the fused policy ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_rollout_with_the_policy_is_step_then_terminate_then_act(dtype):
    """The reference loop and the option-off rollout run the policy as dm_policy_act's launch; the horizon kernel's in-wave policy step forms every sum in that
    launch's order (csrc/policy_wave_launch_order.h), so actions and values are equal bit for bit, not to float32 rounding."""
    n, Tn = 48, 4
    idx, q, v = HC.states(n)
    pol, W = GB.fused_policy()
    a0 = HC.actions(1, n)[0]
    res = {}
    for how in ("reference", "off", "on"):
        env = make(n, how == "on", step_queue=8, dtype=dtype)
        b = env.batch
        start(b, idx, q, v)
        ac, ob, rew, dn, vp = horizon_rows(Tn, n, a0=a0)
        if how == "reference":
            for t in range(Tn):
                b.step(ac[t], 1, (ob[t], rew[t], dn[t])); b.join()
                pol._counter = 7 + t - 1
                pol.act(True, ob[t], out=ac[t + 1], vpred_out=vp[t])
        else:
            b.rollout(ac, (ob, rew, dn), 1, W, vp, True, pol._seed, 7)
        res[how] = result(b, (ac, ob, rew, dn, vp), STATE)
        env.close()
    assert res["reference"]["rows3"].sum() >= 4 and res["reference"]["rows3"][0].sum() < n      # some episodes ended, by no means all
    check_inputs(n, res["reference"]["rows0"][:Tn], idx, q, v, res["reference"]["rows3"], want_mix=False, dtype=dtype)
    if dtype == 64:
        assert_same(res["off"], res["reference"])
    # (float32: MlpPolicy.act is the float64 library's policy launch, the rollout's the float32 library's own — another build of the same kernel, so the
    #  hand-written loop is no reference there; the option-off rollout is)
    assert_same(res["on"], res["off"])


# ---- the step queue ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [2, True])
def test_step_queue_runs_one_horizon_launch_with_termination_inside(packed):
    n = 66
    idx, q, v = HC.states(n)
    act = HC.actions(STEPS, n)
    res = []
    for on in (False, True):
        env = make(n, on, step_queue=8, reward="imitation", packed=packed)
        b = env.batch
        start(b, idx, q, v)
        keep = []
        queued_steps(b, act, 0, STEPS, keep=keep)
        stats = b.queue_stats()
        assert (stats[0] >= 1 and stats[1] == STEPS) if on else stats == (0, 0, 0)
        res.append(stacked(b, keep, STATE, actions=False))
        env.close()
    check_inputs(n, act, idx, q, v, res[0]["rows2"], reward="imitation", packed=packed)
    assert_same(res[1], res[0], packed)


# ---- the truncation log ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [2, True])
def test_truncation_log_and_ticks(packed):
    n = 66
    idx, q, v = HC.states(n)
    act = HC.actions(2 * STEPS, n)
    logs = []
    for on in (False, True):
        env = make(n, on, fall=None, log=n * 6, packed=packed)                            # (n * 3 records per horizon: two horizons without clearing)
        b = env.batch
        start(b, idx, q, v)
        first = horizon_rows(STEPS, n, act=act[:STEPS])
        b.rollout(first[0], first[1:4], 1)
        one = truncation_log(b, clear=False)
        second = horizon_rows(STEPS, n, act=act[STEPS:])
        b.rollout(second[0], second[1:4], 1)                               # the log was not cleared: the ticks go on at STEPS
        two = truncation_log(b, clear=True)
        logs.append((one, two, result(b, second[:4], STATE)))
        env.close()
    (one0, two0, res0), (one1, two1, res1) = logs
    assert one0[0] >= n // 2 and {2, 5} <= set(one0[1][:, 1].tolist()) and one0[1][:, 1].max() < STEPS
    later = two0[1][two0[1][:, 1] >= STEPS]
    assert len(later) >= n // 2 and two0[0] == one0[0] + len(later) and later[:, 1].max() < 2 * STEPS
    for x, y in zip(one1 + two1, one0 + two0):                             # counts, {env, tick, frame_idx, frame_init} rows, qpos, qvel
        assert_same({"x": np.asarray(x)}, {"x": np.asarray(y)}, packed)
    assert_same(res1, res0, packed)


def test_collector_bootstrap_values_do_not_depend_on_the_option():
    """the collector's fused segment is a closed loop through the policy: equal because the horizon kernel's policy step is the policy launch's arithmetic"""
    n, Tn = 48, 8
    segs = []
    for on in (False, True):
        env = DPVecEnv(n, motion="walk", autoreset="init", seed=SEED, packed=2, max_episode_steps=LIMIT, horizon_termination=on)
        pi = MlpPolicy(device=DEV, seed=3); pi.seed(4)
        c = SegmentCollector(pi, env, Tn, fused=True, bootstrap_time_limit=True)
        c.launch()
        seg = c.collect()
        segs.append({k: seg[k].cpu().numpy() for k in ("ob", "rew", "vpred", "new", "ac", "vboot")})
        assert seg.trunc_count() >= n // 2
        env.close()
    assert np.count_nonzero(segs[0]["vboot"]) >= n // 2
    for k in segs[0]:
        np.testing.assert_array_equal(segs[1][k], segs[0][k], err_msg=k)


# ---- off after on --------------------------------------------------------------------------------------------------------------------------------------
def test_option_off_after_on_restores_step_launches():
    n = 66
    idx, q, v = HC.states(n)
    act = HC.actions(2 * STEPS, n)
    res = []
    for toggled in (False, True):
        env = make(n, toggled, step_queue=8)
        b = env.batch
        start(b, idx, q, v)
        keep = []
        queued_steps(b, act, 0, STEPS, keep=keep)
        s1 = b.queue_stats()
        if toggled:
            b.set_option(A.OPT_HORIZON_TERMINATION, 0)
        queued_steps(b, act, STEPS, 2 * STEPS, keep=keep)
        s2 = b.queue_stats()
        assert (s1[0] >= 1 and s1[1] == STEPS) if toggled else s1 == (0, 0, 0)
        assert s2 == s1                                                    # with the option off (again) nothing is queued: step launches
        res.append(stacked(b, keep, STATE, actions=False))
        env.close()
    check_inputs(n, act, idx, q, v, res[0]["rows2"], want_mix=False)
    assert_same(res[1], res[0])
