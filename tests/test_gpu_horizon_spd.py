"""Action modes 3 ("spd-target") and 4 ("spd-mocap") inside the horizon launch and the step queue (DM_OPT_HORIZON_SPD; csrc/kernels_rollout_spd.hip) on the GPU.

The reference is always the same build's own path with the option OFF — step launches with the controller in the per-step kernels — on the same batch
configuration, and the comparison is bit for bit: every output row, the state fields (DM_F_CTRL among them), the counters.  The per-step kernel of both
twins is, for bit identity, the packed one with the three-set code (packed=2, DM_OPT_PACKED = 2): a horizon's waves call that instantiation for an
environment near the two-set capacity, so an environment at 33 .. 40 rows stays on the packed path in both forms.  The termination comparison runs once
more with packed=True (DM_OPT_PACKED 1), where the step launches hand such an env-step to the one-env code: discrete arrays equal, float arrays within
4x a deviation the test measures itself between two paths that differ on exactly those env-steps (see there)."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
from deepmimic_mujoco_amd import termination as TM
from deepmimic_mujoco_amd.rollout import SegmentCollector
from tests import helpers as H
from tests import horizon_term_cases as HC
from tests import spd_numpy as S
from tests import gpu_batch as GB
from tests.gpu_batch import DEV, assert_bits, horizon_rows, queued_steps, result, stacked, start

pytestmark = pytest.mark.gpu
SEED = 5
TOL = 1e-9                    # the bar of tests/test_gpu_spd.py against the restatement
MODE_NAME = {3: "spd-target", 4: "spd-mocap"}
DEEPMIMIC = TM.fall_body_mask("deepmimic")
STATE = GB.STATE + (A.F_CTRL,)
TERM_STATE = STATE + GB.TERM_FIELDS


def make(n, mode, on, reward="imitation", autoreset=None, nsub=1, dtype=64, packed=2, step_queue=0, fall=None, limit=0, horizon_termination=False):
    env = DPVecEnv(n, motion="walk", reward=reward, autoreset=autoreset, seed=SEED, dtype=dtype, packed=packed, step_queue=step_queue, frame_skip=nsub,
                   action_mode=MODE_NAME[mode], horizon_spd=on, fall_contact_bodies=fall, max_episode_steps=limit, horizon_termination=horizon_termination)
    assert env.packed and env.horizon_spd == on and env.batch.options.get(A.OPT_HORIZON_SPD, 0) == (1 if on else 0)
    return env


# (the action seeds are those at which the inputs hold horizon_against_steps' input condition in every case of the grid: 3 does not in mode 4 with 2 substeps
#  under "alive" — env 7 lands at 35 rows from 0 in step 10 —, 4 does; the float32 library's case has its own trajectory and its own seed)
STATE_SEED, ACTION_SEED, ACTION_SEED32 = 8, 4, 3


def many_row_inputs(n, mode, T, action_seed=None):
    """helpers.varied_states with two many-row states (more than 40 constraint rows: the packed step hands them to the one-env code), placed as in
    tests/test_gpu_spd.py, and open-loop actions: mode 3 target poses around the starting frames, mode 4 offsets"""
    idx, q, v, _ws, _c = H.varied_states(n, seed=STATE_SEED)
    hi, hq, hv = HC.many_rows()
    for e, k in ((1, 0), (n - 3, -1)):
        q[e], v[e], idx[e] = hq[k], hv[k], hi[k]
    off = 0.2 * np.random.RandomState(ACTION_SEED if action_seed is None else action_seed).randn(T, n, 28)
    return idx, q, v, (H.mocap().data_config[idx][None, :, 7:] + off if mode == 3 else off)


# ---- the option --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_option_values(dtype):
    env = DPVecEnv(4, dtype=dtype, action_mode="spd-target")
    b = env.batch
    for v in (1, 0, 1, 0):
        b.set_option(A.OPT_HORIZON_SPD, v)
    for bad in (2, -1):
        with pytest.raises(A.DmenvError, match="DM_OPT_HORIZON_SPD"):
            b.set_option(A.OPT_HORIZON_SPD, bad)
    assert b.options[A.OPT_HORIZON_SPD] == 0
    env.close()


# ---- one launch per horizon against step launches ------------------------------------------------------------------------------------------------
def horizon_against_steps(mode, nsub, reward, dtype, action_seed=None):
    """n = 13 (a last wave with spare slots), T = 12.  Off: T unqueued step launches (queue depth set, nothing queued).  On: the same calls, queued and run as
    ONE horizon launch; and dm_batch_rollout on a third batch.
    Input condition.  A horizon's wave picks the lean or the three-set step from its environments' row counts after the previous step, and an env-step that
    lands at 33 .. 40 rows from a wave predicted lean is re-stepped by the one-env code, where packed=2's step launches keep it on the three-set code: other
    sums, by design, in action modes 0..2 too (slot_rollout `heavy`).  The inputs hold no such env-step: every form re-steps the same number of env-steps."""
    n, T = 13, 12
    idx, q, v, act = many_row_inputs(n, mode, T, action_seed)
    res, redo, rows = {}, {}, [np.zeros(n, dtype=np.int32)]
    for how in ("off", "queue", "rollout"):
        env = make(n, mode, how != "off", reward=reward, nsub=nsub, dtype=dtype, step_queue=16 if how != "rollout" else 0)
        b = env.batch
        start(b, idx, q, v)
        redo0 = b.redo_total()
        if how == "rollout":
            bufs = horizon_rows(T, n, act=act)
            b.rollout(bufs[0], bufs[1:4], nsub)
            res[how] = result(b, bufs[:4], STATE)
            res[how]["rows0"] = res[how]["rows0"][:T]
        else:
            keep = []
            if how == "off":
                rows[0] = b.get(A.F_NEFC).copy()
            queued_steps(b, act, 0, T, nsub, keep, (lambda t: rows.append(b.get(A.F_NEFC).copy())) if how == "off" else None)
            assert b.queue_stats() == ((1, T, 0) if how == "queue" else (0, 0, 0))
            res[how] = stacked(b, keep, STATE)
        redo[how] = b.redo_total() - redo0
        env.close()
    print("mode %d, %d substeps, %s, float%d: env-steps re-stepped by the one-env code: %s; constraint rows after every step launch (step x env):\n%s"
          % (mode, nsub, reward, dtype, redo, np.stack(rows)))
    assert min(redo.values()) > 0, "the many-row states must be re-stepped by the one-env code"
    assert redo["queue"] == redo["rollout"] == redo["off"], "input condition: an env-step the horizon's waves predicted lean landed at 33 .. 40 rows"
    assert np.isfinite(res["off"]["rows1"]).all()
    assert_bits(res["queue"], res["off"])
    assert_bits(res["rollout"], res["off"])


@pytest.mark.parametrize("reward", ["imitation", "alive"])
@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("mode", [3, 4])
def test_rollout_equals_step_launches(mode, nsub, reward):
    horizon_against_steps(mode, nsub, reward, 64)


def test_rollout_equals_step_launches_on_the_float32_library():
    horizon_against_steps(4, 2, "imitation", 32, ACTION_SEED32)


WEIGHTS_STATE_SEED = 10        # (episodes end inside the horizon in both modes)


def weights_case(mode, stochastic=True):
    """the closed loop through the fused policy step from exact mocap frames, both forms -> (results, env-steps re-stepped) per form"""
    n, T, nsub = 13, 12, 2
    mc = H.mocap()
    idx = np.random.RandomState(WEIGHTS_STATE_SEED).randint(0, mc.data_config.shape[0], size=n).astype(np.int32)
    q, v = mc.data_config[idx].copy(), mc.data_vel[idx].copy()
    a0 = mc.data_config[idx][:, 7:] if mode == 3 else np.zeros((n, 28))
    pol, W = GB.fused_policy()
    res, redo = {}, {}
    for how in ("step_act", "on"):
        env = make(n, mode, how == "on", nsub=nsub)
        b = env.batch
        start(b, idx, q, v)
        redo0 = b.redo_total()
        ac, ob, rew, dn, vp = horizon_rows(T, n, a0=a0)
        if how == "on":
            b.rollout(ac, (ob, rew, dn), nsub, W, vp, stochastic, pol._seed, 7)
        else:
            for t in range(T):
                b.step_act(ac[t], nsub, (ob[t], rew[t], dn[t]), W, ac[t + 1], vp[t], stochastic, pol._seed, 7 + t)
        res[how] = result(b, (ac, ob, rew, dn, vp), STATE)
        redo[how] = b.redo_total() - redo0
        env.close()
    return res, redo


@pytest.mark.parametrize("mode", [3, 4])
def test_rollout_with_weights_equals_step_act_calls(mode):
    """the horizon's in-wave policy step is the one the step launches of these modes fuse (k_step_packed_act_spd): action and value rows bit for bit.
    Input condition: no environment is re-stepped by the one-env code in either form — such an environment gets its policy step from the one-env code's
    epilogue in a step launch and from its wave's four-environment epilogue in a horizon launch, the same MLP summed in another order, in every action
    mode (tests/test_gpu_rollout.py test_horizon_launch_equals_step_by_step)."""
    res, redo = weights_case(mode)
    print("mode %d: env-steps re-stepped by the one-env code: %s" % (mode, redo))
    assert redo == {"step_act": 0, "on": 0}, "input condition: no re-stepped environment"
    assert np.isfinite(res["on"]["rows0"]).all() and np.abs(res["on"]["rows4"]).max() > 0
    assert_bits(res["on"], res["step_act"])


@pytest.mark.parametrize("mode", [3, 4])
def test_rollout_matches_the_restatement(mode):
    """the option-on rollout in lock step with tests/spd_numpy.py on the CPU oracle, at the bars of tests/test_gpu_spd.py (reward mode 1: the frame cursor that
    mode 4 reads moves; auto-reset off; 2 substeps)"""
    from oracle import oracle as O
    n, T, nsub = 13, 15, 2
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    h = float(om.get("timestep")[0])
    idx, q, v, _ws, _c = H.varied_states(n, seed=5)
    off = 0.2 * np.random.RandomState(1).randn(T, n, 28)
    act = mc.data_config[idx][None, :, 7:] + off if mode == 3 else off
    env = make(n, mode, True, reward="v3-config", nsub=nsub, packed=True)
    b = env.batch
    start(b, idx, q, v)
    bufs = horizon_rows(T, n, act=act)
    b.rollout(bufs[0], bufs[1:4], nsub)
    r = result(b, bufs[1:4], STATE)
    env.close()
    ob, rew, dn = r["rows0"], r["rows1"], r["rows2"]
    fidx = idx.astype(np.int64).copy()
    worst, worst_ctrl, ods = 0.0, 0.0, []
    for e in range(n):
        od = O.Data(om); od.reset(); od.set_state(q[e], v[e]); ods.append(od)
    for t in range(T):
        for e in range(n):
            o, rr, d, nxt, c = S.env_step(cm, ods[e], mode, act[t, e], mc, int(fidx[e]), nsub, h, reward_mode=1)
            fidx[e] = nxt
            worst = max(worst, H.rel_err(ob[t, e], o), abs(rew[t, e] - rr) / max(1.0, abs(rr)))
            assert bool(dn[t, e]) == d, (t, e)
            if t == T - 1:
                worst_ctrl = max(worst_ctrl, H.rel_err(r[A.F_CTRL][e], c))
    print("horizon launch, mode %d: worst rel err obs / reward %.3e, last ctrl %.3e" % (mode, worst, worst_ctrl))
    assert worst < TOL and worst_ctrl < TOL
    assert np.array_equal(r[A.F_FRAME_IDX], fidx.astype(np.int32))
    for e in range(n):
        assert H.rel_err(r[A.F_QPOS][e], ods[e].get("qpos")) < TOL
        assert H.rel_err(r[A.F_QACC_WARMSTART][e], ods[e].get("qacc_warmstart")) < max(TOL, 1e-8)
        assert abs(r[A.F_TIME][e] - ods[e].get("time")[0]) < 1e-12


# ---- the step queue ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4])
def test_step_queue_queues_again(mode):
    """step_queue=8, 12 calls: the calls are queued (nothing launches until the eighth is followed by a ninth), and the results are the unqueued run's"""
    n, T, nsub = 66, 12, 2
    idx, q, v, act = many_row_inputs(n, mode, T)
    res = []
    for queue in (0, 8):
        env = make(n, mode, True, autoreset="rsi", nsub=nsub, step_queue=queue)
        b = env.batch
        start(b, idx, q, v)
        keep = []
        seen = queued_steps(b, act, 0, T, nsub, keep)
        if queue:
            assert seen == [(0, 0, t + 1) for t in range(8)] + [(1, 8, t - 7) for t in range(8, T)]
            assert b.queue_stats() == (2, T, 0)
        else:
            assert seen == [(0, 0, 0)] * T
        res.append(stacked(b, keep, STATE))
        env.close()
    assert res[0]["rows3"].sum() >= 1                                       # an auto-reset inside the horizon
    assert_bits(res[1], res[0])


# ---- with early termination inside -------------------------------------------------------------------------------------------------------------------
def term_cfg(mode, packed):
    return dict(mode=mode, reward="imitation", autoreset="rsi", nsub=1, packed=packed, fall="deepmimic", limit=3)


def term_rollout(n, T, on, idx, q, v, act, W=None, pol=None, **cfg):
    mode = cfg.pop("mode")
    env = make(n, mode, on, horizon_termination=on, **cfg)
    b = env.batch
    start(b, idx, q, v)
    if W is None:
        bufs = horizon_rows(T, n, act=act)
        b.rollout(bufs[0], bufs[1:4], cfg["nsub"])
        r = result(b, bufs[:4], TERM_STATE)
    else:
        bufs = horizon_rows(T, n, a0=act[0])
        b.rollout(bufs[0], bufs[1:4], cfg["nsub"], W, bufs[4], True, pol._seed, 7)
        r = result(b, bufs, TERM_STATE)
    stats = b.queue_stats()
    env.close()
    return r, stats


def check_fall_decisions(n, act, idx, q, v, done_rows, **cfg):
    """the input condition (tests/test_gpu_horizon_termination.py): from the states the reference's own steps leave ahead of termination — a probe batch without
    termination stepped from the reference's state, step by step — no fall decision lies within HC.BOUNDARY of the rule's boundary"""
    cm = H.compiled_model()
    mode = cfg.pop("mode")
    pre_q, stepdone = GB.states_before_termination(lambda: make(n, mode, False, **cfg), lambda: make(n, mode, False, **dict(cfg, fall=None, limit=0)),
                                                   idx, q, v, act, cfg["nsub"])
    closest = HC.closest_decision(cm, pre_q, ~stepdone, TM.geoms_of_bodies(DEEPMIMIC, cm.geom_bodyid))
    ended = (done_rows != 0) & ~stepdone
    print("closest fall decision %.3e m from its boundary; %d ended by the step, %d by termination, %d env-steps went on" % (closest, stepdone.sum(), ended.sum(), (done_rows == 0).sum()))
    assert closest > HC.BOUNDARY
    assert ended.any() and (done_rows == 0).any()


@pytest.mark.parametrize("policy", [False, True])
@pytest.mark.parametrize("mode", [3, 4])
def test_termination_inside_equals_step_terminate_act(mode, policy):
    """both options on against step launches, each followed by the termination launch and — with weights — dm_policy_act: packed=2, bit for bit, STATE
    fields, reasons and counters included"""
    n, T = 10, 7
    idx, q, v = HC.states(n)
    act = HC.actions(T, n)
    pol, W = GB.fused_policy() if policy else (None, None)
    cfg = term_cfg(mode, 2)
    ref, s0 = term_rollout(n, T, False, idx, q, v, act, W, pol, **dict(cfg))
    got, _s1 = term_rollout(n, T, True, idx, q, v, act, W, pol, **dict(cfg))
    assert s0 == (0, 0, 0)
    check_fall_decisions(n, ref["rows0"][:T], idx, q, v, ref["rows3"], **dict(cfg))
    assert_bits(got, ref)


@pytest.mark.parametrize("mode", [3, 4])
def test_termination_inside_with_the_lean_step_kernel(mode):
    """packed=True (DM_OPT_PACKED 1).  An env-step at 33 .. 40 rows is the packed three-set code's in any horizon launch and the one-env code's in DM_OPT_PACKED 1's
    step launches: discrete arrays equal; float arrays within 4x the deviation measured here between two parent-commit paths that differ on exactly those
    env-steps — the same inputs through step launches under DM_OPT_PACKED 1 and under 2, option off (the factor: the difference propagates through other steps).
    A measured deviation of 0 requires equality."""
    n, T = 10, 7
    idx, q, v = HC.states(n)
    act = HC.actions(T, n)
    lean, _ = term_rollout(n, T, False, idx, q, v, act, **term_cfg(mode, True))
    ext, _ = term_rollout(n, T, False, idx, q, v, act, **term_cfg(mode, 2))
    got, _ = term_rollout(n, T, True, idx, q, v, act, **term_cfg(mode, True))
    check_fall_decisions(n, act, idx, q, v, lean["rows3"], **term_cfg(mode, True))

    def deviation(x, y):
        worst = 0.0
        for k in y:
            if y[k].dtype.kind == "f":
                assert np.isfinite(x[k]).all()
                worst = max(worst, float((np.abs(x[k] - y[k]) / np.maximum(1.0, np.abs(y[k]))).max()))
        return worst
    for k in lean:
        if lean[k].dtype.kind in "iub":
            np.testing.assert_array_equal(ext[k], lean[k], err_msg="step launches, DM_OPT_PACKED 2 against 1: %s" % k)
            np.testing.assert_array_equal(got[k], lean[k], err_msg=str(k))
    measured, seen = deviation(ext, lean), deviation(got, lean)
    print("mode %d, DM_OPT_PACKED 1: step launches under 2 against 1 deviate by %.3e; the horizon launch against the step launches by %.3e (relative to max(1, |x|))"
          % (mode, measured, seen))
    assert seen <= 4 * measured


# ---- the collector -------------------------------------------------------------------------------------------------------------------------------------
def test_collector_segment_does_not_depend_on_the_option():
    n, Tn = 256, 8
    segs, rates = [], []
    for on in (False, True):
        env = DPVecEnv(n, action_mode="spd-mocap", reward="imitation", packed=2, horizon_spd=on, seed=SEED)
        pi = MlpPolicy(device=DEV, seed=3); pi.seed(4)
        c = SegmentCollector(pi, env, Tn, fused=True)
        redo0 = env.batch.redo_total()
        c.launch()
        seg = c.collect()
        segs.append({k: seg[k].cpu().numpy() for k in ("ob", "rew", "vpred", "new", "ac")})
        rates.append((env.batch.redo_total() - redo0) / float(Tn * n))         # what HorizonKernelChoice reads: the launch feeds dm_batch_redo_total as the plain one does
        why = env.batch.redo_reasons()
        assert sum(why[1:]) >= why[0] >= redo0                                  # ... and its reasons' tallies
        env.close()
    print("re-stepped env-steps per env-step: step launches %.4f, horizon launch %.4f" % tuple(rates))
    assert 0.0 <= rates[0] <= rates[1] <= 1.0                                  # (a horizon's waves predict which step to call: a miss is re-stepped too)
    assert np.isfinite(segs[0]["ob"]).all()
    for k in segs[0]:
        np.testing.assert_array_equal(segs[1][k], segs[0][k], err_msg=k)


def test_horizon_kernel_choice_reads_the_overflow_rate_of_an_spd_horizon():
    """an env that leaves the kernel to the collector (packed=None, 256 envs): HorizonKernelChoice starts packed, the horizon is one launch under the option, and
    the rate it reads before the second horizon is the first one's re-stepped share"""
    n, Tn = 256, 8
    env = DPVecEnv(n, action_mode="spd-mocap", reward="imitation", horizon_spd=True, seed=SEED)
    assert env.horizon_packed_ok
    pi = MlpPolicy(device=DEV, seed=3); pi.seed(4)
    c = SegmentCollector(pi, env, Tn, fused=True)
    redo0 = env.batch.redo_total()
    c.launch(); c.collect()
    first = env.batch.redo_total() - redo0
    c.launch(); c.collect()
    k = c.kernel_choice
    print("re-stepped share of the first horizon: %s (%d env-steps)" % (k.last_redo_rate, first))
    assert k.packed_now is True and k.last_redo_rate == first / float(Tn * n) and 0.0 <= k.last_redo_rate <= k.REDO_RATE_MAX
    env.close()


# ---- off after on --------------------------------------------------------------------------------------------------------------------------------------
def test_option_off_after_on_restores_step_launches():
    n, T, mode, nsub = 66, 6, 4, 1
    idx, q, v, act = many_row_inputs(n, mode, 2 * T)
    res = []
    for toggled in (False, True):
        env = make(n, mode, toggled, step_queue=8, nsub=nsub)
        b = env.batch
        start(b, idx, q, v)
        keep = []
        queued_steps(b, act, 0, T, nsub, keep)
        s1 = b.queue_stats()
        if toggled:
            b.set_option(A.OPT_HORIZON_SPD, 0)
        seen = queued_steps(b, act, T, 2 * T, nsub, keep)
        assert s1 == ((1, T, 0) if toggled else (0, 0, 0))
        assert seen == [s1] * T                                            # with the option off (again) nothing is queued: step launches
        res.append(stacked(b, keep, STATE))
        env.close()
    assert_bits(res[1], res[0])
