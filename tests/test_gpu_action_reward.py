"""Every action mode with every reward mode on the device, through the C ABI: the two bodies of source (one env per wave, four per wave)
against the float64 rows of tests/action_reward_cases.py, every other launch form against the packed form bit for bit, the fused-policy forms
against the reference through the action rows they report, DPVecEnv past the clip's last frame, and the float32 library.
tests/test_action_reward.py runs the pairs with reward modes 2 and 4 on the wave testbench and says what they pin.

Bars.  float64 library: helpers.compare_rollout's (1e-9 relative; the warm start 1e-8).  Measured on an MI355X, worst relative error
(helpers.rel_err) over the pairs, every test printing its own pair's:
    form                       DM_F_CTRL   obs       reward    final qpos   qacc_warmstart
    narrow      (20 pairs)     5.9e-14     6.2e-14   4.8e-15   7.2e-15      1.7e-13
    packed      (20 pairs)     5.5e-14     1.5e-13   4.8e-15   6.8e-15      2.0e-13
    narrow / packed, reward 4 with two substeps   9.9e-14 / 3.4e-14   1.2e-13 / 4.1e-14   4.6e-14 / 1.6e-14   2.6e-14 / 9.6e-15   6.7e-14 / 7.8e-14
    narrow-act  (8 pairs)      6.1e-14     2.9e-13   4.8e-15   1.5e-14      1.5e-12
    packed-act  (8 pairs)      5.7e-14     2.8e-13   5.3e-15   1.4e-14      1.5e-12
    rollout-act (8 pairs)      5.7e-14     2.8e-13   5.3e-15   1.4e-14      1.5e-12
Action mode 2 has the largest figures in every form (its gains multiply the state's rounding), mode 1 the smallest (DM_F_CTRL 1e-15)."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch, DPVecEnv
from tests import action_reward_cases as AR
from tests import float32_cases as F32
from tests import helpers as H
from tests import gpu_batch as GB

pytestmark = pytest.mark.gpu
TOL = 1e-9
N = 13                                    # three full packed waves and one with three spare slots
ACTIONS, REWARDS = (1, 2, 3, 4), (0, 1, 2, 3, 4)
UNCOVERED = [(am, rm) for am in ACTIONS for rm in (2, 4)]      # the pairs of tests/test_action_reward.py

# the launch forms of tests/gpu_batch.py run here ("rollout", "queue": a horizon launch in action modes 1 and 2, step launches in 3 and 4)
FORMS = {k: GB.FORMS[k] for k in ("narrow", "packed", "packed-ext", "rollout", "queue", "narrow-act", "packed-act", "rollout-act")}
_PACKED = {}


def _make(case, packed, dtype=64):
    mc = H.mocap()
    imit = AR.imit_inputs() if case["reward_mode"] >= 3 else None
    b = Batch(H.compiled_model(), mc.data_config, mc.data_vel, case["n"], device=0, mocap_dt=float(mc.dt), imitation=imit, dtype=dtype)
    b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_ACTION_MODE, case["action_mode"]); b.set_option(A.OPT_REWARD_MODE, case["reward_mode"])
    return b


def _run(form, case):
    """The case through one launch form -> (what the form produced, as action_reward_cases.check takes it; the action rows it consumed)."""
    lf = FORMS[form]
    n, T, nsub = case["n"], case["T"], case["nsub"]
    b = _make(case, lf.packed)
    if lf.issue == "step" and not lf.policy:
        got = AR.run_steps(b, case)
        b.close()
        return got, case["acts"]
    AR.prepare(b, case)
    ac, ob, rew, dn, vp = GB.horizon_rows(T, n, act=case["acts"]); ac[T] = ac[T - 1]   # open loop: every row given; with a policy rows 1.. are overwritten
    pol, W = GB.fused_policy() if lf.policy else (None, None)
    got = dict(ctrl=[None] * T, cursors=[None] * T)

    def between(t):
        if lf.issue == "queue":             # nothing read from the batch: every call stays queued
            got["queued"] = b.queue_stats()
        else:
            got["ctrl"][t] = b.get(A.F_CTRL); got["cursors"][t] = b.get(A.F_FRAME_IDX)
    GB.issue_steps(b, lf, ac, ob, rew, dn, nsub, pol=pol, W=W, vp=vp, between=between)
    got["queue_stats"] = b.queue_stats()
    got["ctrl"][T - 1] = b.get(A.F_CTRL); got["cursors"][T - 1] = b.get(A.F_FRAME_IDX)
    got.update(obs=ob.cpu().numpy(), reward=rew.cpu().numpy(), done=dn.cpu().numpy(), init=b.get(A.F_FRAME_INIT), qpos=b.get(A.F_QPOS),
               qvel=b.get(A.F_QVEL), qacc_warmstart=b.get(A.F_QACC_WARMSTART), time=b.get(A.F_TIME))
    acts = ac.cpu().numpy()[:T]
    b.close()
    return got, acts


def _packed(case):
    key = (case["action_mode"], case["reward_mode"], case["nsub"])
    if key not in _PACKED:
        _PACKED[key] = _run("packed", case)[0]
    return _PACKED[key]


@pytest.mark.parametrize("form", ["narrow", "packed"])
@pytest.mark.parametrize("rm", REWARDS)
@pytest.mark.parametrize("am", ACTIONS)
def test_every_pair_matches_the_reference(am, rm, form):
    """13 envs, 4 steps: DM_F_CTRL and DM_F_FRAME_IDX after every step, obs / reward / done every step, DM_F_FRAME_INIT, the final qpos /
    qacc_warmstart / time — every env of the batch."""
    case = AR.make_case(am, rm, n=N)
    got = _packed(case) if form == "packed" else _run(form, case)[0]
    worst = AR.check(case, AR.expected(case), got, tol=TOL)
    print("device action %d reward %d %s: worst rel err %s" % (am, rm, form, {k: "%.1e" % x for k, x in worst.items()}))


@pytest.mark.parametrize("am", ACTIONS)
def test_v1_reward_with_two_substeps_matches_the_reference(am):
    """reward mode 4 with two substeps: the update interval of the frame rule is 1 instead of 2 (asserted), on both bodies of source"""
    assert AR.upd_of(4, 2) != AR.upd_of(4, 1)
    case = AR.make_case(am, 4, nsub=2, n=N)
    for form in ("narrow", "packed"):
        worst = AR.check(case, AR.expected(case), _run(form, case)[0], tol=TOL)
        print("device action %d reward 4, two substeps, %s: worst rel err %s" % (am, form, {k: "%.1e" % x for k, x in worst.items()}))


@pytest.mark.parametrize("rm", REWARDS)
@pytest.mark.parametrize("am", ACTIONS)
def test_every_other_form_equals_packed_bit_for_bit(am, rm):
    """packed-ext, dm_batch_rollout and DM_OPT_STEP_QUEUE against the packed per-step launches: rows, both cursors, the final state and the last
    DM_F_CTRL, bit for bit, on the envs whose largest REFERENCE row count over the run's RK evaluations is at most 32 (chosen by the oracle alone;
    above that the forms legitimately run different code: the redo kernel against the three-set code); the other envs against the reference."""
    case = AR.make_case(am, rm, n=N)
    exp = AR.expected(case)
    envs = [e for e in range(N) if exp["peak"][e] <= 32]
    assert len(envs) >= 10, exp["peak"]
    ref = _packed(case)
    for form in ("packed-ext", "rollout", "queue"):
        got, _acts = _run(form, case)
        AR.same_bits(got, ref, envs)
        AR.check(case, exp, got, tol=TOL)
        if form == "queue":                 # a horizon launch for the modes whose front end lives in it, the documented fall-back for the others
            assert got["queued"] == ((0, 0, case["T"]) if am <= 2 else (0, 0, 0)), got["queued"]
            assert got["queue_stats"] == ((1, case["T"], 0) if am <= 2 else (0, 0, 0)), got["queue_stats"]


@pytest.mark.parametrize("am,rm", UNCOVERED)
def test_fused_policy_forms_match_the_reference_on_their_own_actions(am, rm):
    """dm_batch_step_act (one env and four envs per wave) and dm_batch_rollout with weights: the policy writes the next action row inside the
    step kernel, so the reference is driven with the rows the form reports."""
    case = AR.make_case(am, rm, n=N)
    for form in ("narrow-act", "packed-act", "rollout-act"):
        got, acts = _run(form, case)
        assert np.array_equal(acts[0], case["acts"][0]) and not np.array_equal(acts[1:], case["acts"][1:]), "rows 1.. are the policy's"
        worst = AR.check(case, AR.expected(case, acts), got, tol=TOL)
        print("device action %d reward %d %s: worst rel err %s" % (am, rm, form, {k: "%.1e" % x for k, x in worst.items()}))


def _front_end_ctrl(case, t, q, v, cursor):
    """The reference rule for DM_F_CTRL of step t (one substep) applied to the state (q, v) and the cursors the batch holds as the step starts."""
    from oracle import oracle as O
    from tests import spd_numpy as S
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    am, rm = case["action_mode"], case["reward_mode"]
    kp, kd = AR.golden_gains()
    out = np.zeros((case["n"], 28))
    od = O.Data(om)
    for e in range(case["n"]):
        k = S.start_frame(rm, int(cursor[e]), int(case["init"][e]), mc.data_config.shape[0], AR.upd_of(rm, 1))
        if am <= 2:
            out[e] = AR.host_ctrl(am, case["acts"][t, e], mc.data_config[k], mc.data_vel[k], q[e], v[e], kp, kd)
        else:
            od.reset(); od.set_state(q[e], v[e])
            out[e] = S.spd_ctrl(cm, od, *S.targets(am, case["acts"][t, e], mc, k), AR.timestep())
    return out


@pytest.mark.parametrize("action_mode", ["p-control", "pd", "spd-target", "spd-mocap"])
@pytest.mark.parametrize("reward", ["v2-pose", "v1-quat"])
def test_dpvecenv_tracks_the_clip_past_its_last_frame(reward, action_mode):
    """DPVecEnv, 8 envs, 45 steps of zero action from an RSI reset, auto-reset off: the cursor passes the 39 frames of `walk`, where the
    front ends used to leave the mocap tables.
    After EVERY step DM_F_CTRL is the reference rule's value for the state and cursors the batch held as that step started (1e-9), and after the
    last step it is the value of the reference stepped in lock step from the reset's state (1e-9) — except that the lock-step figure of "pd" is
    printed, not asserted: the explicit PD torque (kp up to 1000 at h = 1/60 s; "spd-mocap" is its stable form for that reason) amplifies
    rounding differences by about 10 every three steps, for any two float64 evaluations.  On the wave testbench, where kernel source and
    reference agree to 1e-13 over the first ten steps, the lock-step DM_F_CTRL of "pd" is off by 4.2e-05 (v2-pose) and 2.8e-07 (v1-quat)
    after step 45, while the other three modes stay at 1.2e-14 or better.  On an MI355X: "pd" 6.9e-05 and 6.2e-07, the other modes 3.9e-14
    or better; against the rule at each step's own start every mode is within 7.3e-15."""
    from deepmimic_mujoco_amd.dp_env import ACTION_MODES, REWARD_MODES
    n, T = 8, 45
    env = DPVecEnv(n, motion="walk", device=0, reward=reward, autoreset=None, seed=3, action_mode=action_mode)
    b = env.batch
    env.reset("rsi")
    assert env.frame_skip == 1
    case = dict(action_mode=ACTION_MODES[action_mode], reward_mode=REWARD_MODES[reward], nsub=env.frame_skip, n=n, T=T, seed=None,
                q=b.get(A.F_QPOS), v=b.get(A.F_QVEL), cursor=b.get(A.F_FRAME_IDX), init=b.get(A.F_FRAME_INIT), acts=np.zeros((T, n, 28)))
    assert np.all(case["cursor"] == 0) and T > b.n_frames
    exp = AR.expected(case, case["acts"])
    worst = 0.0
    for t in range(T):
        q, v, cursor = b.get(A.F_QPOS), b.get(A.F_QVEL), b.get(A.F_FRAME_IDX)
        assert np.all(cursor == t)
        obs, rew, done, _info = env.step(case["acts"][t])
        want = _front_end_ctrl(case, t, q, v, cursor)
        worst = max(worst, max(H.rel_err(b.get(A.F_CTRL)[e], want[e]) for e in range(n)))
    assert np.array_equal(b.get(A.F_FRAME_IDX), exp["cursor"][T]) and np.all(exp["cursor"][T] == T)
    err = max(H.rel_err(b.get(A.F_CTRL)[e], exp["ctrl"][T - 1, e]) for e in range(n))
    print("DPVecEnv %s / %s, %d steps: DM_F_CTRL against the rule at each step's own start %.2e; after the last step against the lock-step reference %.2e (obs %.2e)"
          % (reward, action_mode, T, worst, err, H.rel_err(obs, exp["obs"][T - 1])))
    env.close()
    assert worst < TOL
    assert err < TOL or action_mode == "pd"


@pytest.mark.parametrize("rm", [2, 4])
@pytest.mark.parametrize("am", [1, 2])
def test_float32_library_front_ends_past_the_last_frame(am, rm):
    """libdmenv32.so, action modes 1 and 2 with reward modes 2 and 4, 13 envs, 4 steps: DM_F_CTRL after every step — the steps at which an env's
    cursor crosses n_frames among them (asserted).  Reference: the float64 host formula on the float32-rounded inputs (the state the float32
    batch holds as the step starts, the rounded mocap rows, gains and action).  Bar: F32.MARGIN = 4 times the error of the same formula evaluated in
    numpy float32, max over the envs against max over the envs, per step.
    Measured, kernel / numpy float32 at the worst step of each: mode 1 9.1e-08 / 6.6e-08 (reward 2), 1.0e-07 / 1.0e-07 (reward 4); mode 2
    1.3e-07 / 9.3e-08 (reward 2), 1.1e-07 / 1.4e-07 (reward 4).  Over all steps the kernel's error is 0.4 .. 1.4 times numpy's: it rounds as numpy
    does, up to FMA contraction inside one expression."""
    case = AR.make_case(am, rm, n=N)
    mc = H.mocap()
    Fr = mc.data_config.shape[0]
    f32 = np.float32
    kp, kd = AR.golden_gains()
    cur, fr = AR.situations(case)
    assert np.any((cur[:-1] < Fr) & (cur[1:] >= Fr)), "no env crosses n_frames between two step starts"
    b = _make(case, 0, dtype=32)
    AR.prepare(b, case)
    worst = (0.0, 0.0)
    for t in range(case["T"]):
        q, v = b.get(A.F_QPOS), b.get(A.F_QVEL)                  # float32 values
        assert np.array_equal(b.get(A.F_FRAME_IDX), cur[t])
        b.step(case["acts"][t], 1)
        ctrl = b.get(A.F_CTRL)
        e_k, e_n = 0.0, 0.0
        for e in range(N):
            k = int(fr[t, e])
            args32 = [x.astype(f32) for x in (case["acts"][t, e], mc.data_config[k], mc.data_vel[k], q[e], v[e], kp, kd)]
            ref = AR.host_ctrl(am, *[x.astype(np.float64) for x in args32])
            np32 = AR.host_ctrl(am, *args32)
            assert np32.dtype == f32
            e_k = max(e_k, H.rel_err(ctrl[e], ref)); e_n = max(e_n, H.rel_err(np32, ref))
        print("float32 action %d reward %d step %d: kernel %.2e, numpy float32 %.2e" % (am, rm, t, e_k, e_n))
        assert e_k <= F32.MARGIN * e_n, (t, e_k, e_n)
        worst = max(worst, (e_k, e_n))
    b.close()
    print("float32 action %d reward %d: worst step kernel %.2e against the envelope %.2e" % (am, rm, worst[0], worst[1]))
