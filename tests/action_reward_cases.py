"""Action modes crossed with reward modes: the float64 expected rows of any (action mode, reward mode, n_substeps) pair (TEST INFRASTRUCTURE).

What is pinned.  The action front ends of modes 1 ("p-control"), 2 ("pd") and 4 ("spd-mocap") track THE MOCAP FRAME THE ENV IS AT AS THE ENV
STEP STARTS (include/dmenv.h DM_OPT_ACTION_MODE).  Reward modes 0, 1 and 3 keep that frame in DM_F_FRAME_IDX; reward modes 2 ("v2-pose") and 4
("v1-quat") keep the reference's two cursors — DM_F_FRAME_IDX counts the episode's steps without bound, the drawn frame sits in DM_F_FRAME_INIT —
and look the frame up as (cursor + init) % F and (cursor // upd + init) % F.  A front end that indexes the mocap tables with the cursor itself
tracks the wrong frame there and, from the episode's F-th step, reads past the tables' end.

The reference.  Nothing is taken from the code under test:
  * ctrl of modes 1 and 2: the host formula on the oracle's own state, gains from tests/golden/env_logic_golden.npz (as
    tests/test_wave_testbench.py test_action_front_ends_on_testbench uses them), fed to the oracle step of the reward mode — Data.env_step for
    reward modes 0..2, env_step_imitation for 3, env_step_v1 for 4;
  * modes 3 and 4: tests/spd_numpy.py's per-substep rule and its env_step (the oracle's epilogue on the state the substeps leave; reward modes 2
    and 4 charge the last substep's unclamped ctrl).

The cursors of a case (reward modes 2 and 4; written after set_state, mirrored into the oracle's idx_curr), so that T = 4 steps contain
  kind 0 (env % 3 == 0): cursor // upd + init wraps modulo F while the cursor itself is far below F (the frame starts at F - 1);
  kind 1 (env % 3 == 1): the cursor itself passes F (cursor = F - 2 or F - 1, init = F - 3) — where the unfixed front ends left the tables;
  kind 2 (env % 3 == 2): an env far from either.
In reward modes 0, 1 and 3 the cursor is the frame set_state was given."""
import numpy as np

from deepmimic_mujoco_amd import _abi as A
from tests import helpers as H
from tests import spd_numpy as S

T_STEPS = 4
_IMIT = {}
_EXPECTED = {}


def imit_inputs(clip="walk"):
    """(table [F, 112], params [32]) of the clip: reward modes 3 and 4"""
    if clip not in _IMIT:
        from deepmimic_mujoco_amd.imitation import ImitationSpec
        _IMIT[clip] = ImitationSpec(H.compiled_model()).table_for(H.mocap(clip))
    return _IMIT[clip]


def timestep():
    return float(H.oracle_model().get("timestep")[0])


def upd_of(reward_mode, nsub):
    return S.update_interval(float(H.mocap().dt), timestep(), nsub) if reward_mode == 4 else 1


def golden_gains():
    g = np.load(H.GOLDEN + "/env_logic_golden.npz")
    return g["kp"], g["kd"]


def host_ctrl(action_mode, action, cfg_row, vel_row, q, v, kp, kd):
    """modes 1 and 2: src/env_torque_test.py:20 and src/mujoco/setting_states.py:207-226; the dtype of the inputs is the dtype of the result"""
    if action_mode == 1:
        return action + cfg_row[7:].dtype.type(0.8) * (cfg_row[7:] - q[7:])
    assert action_mode == 2
    return action + kp * (cfg_row[7:] - q[7:]) + kd * (vel_row[6:] - v[6:])


def cursors(reward_mode, idx, nsub):
    """(cursor [n], init [n]) a case starts from; `idx`: the frames of H.varied_states"""
    n = len(idx)
    F = H.mocap().data_config.shape[0]
    if reward_mode not in (2, 4):
        return idx.astype(np.int32).copy(), idx.astype(np.int32).copy()
    upd = upd_of(reward_mode, nsub)
    cur = np.zeros(n, dtype=np.int32); init = np.zeros(n, dtype=np.int32)
    for e in range(n):
        kind = e % 3
        if kind == 0:
            cur[e] = 8 + e; init[e] = F - 1 - cur[e] // upd
        elif kind == 1:
            cur[e] = F - 2 + (e // 3) % 2; init[e] = F - 3
        else:
            cur[e] = 3 + e; init[e] = 5 + e
    return cur, init


def make_case(action_mode, reward_mode, nsub=1, n=4, T=T_STEPS, seed=5):
    idx, q, v, _ws, _c = H.varied_states(n, seed=seed)
    mc = H.mocap()
    F = mc.data_config.shape[0]
    cur, init = cursors(reward_mode, idx, nsub)
    rng = np.random.RandomState(100 * action_mode + 10 * reward_mode + nsub)
    if action_mode in (1, 2):
        acts = 0.1 * rng.randn(T, n, 28)                       # a motor command on top of the feedback term
    elif action_mode == 3:
        k0 = [S.start_frame(reward_mode, int(cur[e]), int(init[e]), F, upd_of(reward_mode, nsub)) for e in range(n)]
        acts = mc.data_config[k0][None, :, 7:] + 0.2 * rng.randn(T, n, 28)      # target poses around the frames the envs are at
    else:
        acts = 0.2 * rng.randn(T, n, 28)                       # offsets to the frame's pose
    return dict(action_mode=action_mode, reward_mode=reward_mode, nsub=nsub, n=n, T=T, seed=seed, q=q, v=v, cursor=cur, init=init, acts=acts)


def situations(case):
    """The frames the front ends must read, [T, n], with the cursors they start from: what a case is made to contain."""
    F = H.mocap().data_config.shape[0]
    upd = upd_of(case["reward_mode"], case["nsub"])
    cur = case["cursor"][None, :] + np.arange(case["T"])[:, None]
    if case["reward_mode"] == 1:
        cur = cur % F
    if case["reward_mode"] == 3:
        cur = np.where(cur >= F, cur - F, cur)
    fr = np.array([[S.start_frame(case["reward_mode"], int(cur[t, e]), int(case["init"][e]), F, upd) for e in range(case["n"])] for t in range(case["T"])])
    return cur, fr


def prepare(b, case):
    """Put a batch (device or testbench) into the case's start: zero warm start and time, the states, the two cursors."""
    H.start(b, case["init"], case["q"], case["v"])
    if case["reward_mode"] in (2, 4):
        assert np.all(b.get(A.F_FRAME_IDX) == 0) and np.array_equal(b.get(A.F_FRAME_INIT), case["init"])
        b.set(A.F_FRAME_IDX, case["cursor"])
    assert np.array_equal(b.get(A.F_FRAME_IDX), case["cursor"]) and np.array_equal(b.get(A.F_FRAME_INIT), case["init"])


def expected(case, acts=None):
    """The oracle's rows for the case; `acts` [T, n, 28]: the actions a form consumed when they are not the case's own (fused policy forms).
    -> dict: ctrl, obs [T, n, .], reward, done [T, n], cursor [T + 1, n], cycle [T + 1, n], qpos, qacc_warmstart [n, .], time [n],
    peak [n] (the largest constraint row count over the run's RK evaluations)."""
    key = None
    if acts is None:
        key = (case["action_mode"], case["reward_mode"], case["nsub"], case["n"], case["T"], case["seed"])
        if key in _EXPECTED:
            return _EXPECTED[key]
        acts = case["acts"]
    from oracle import oracle as O
    am, rm, nsub, n, T = case["action_mode"], case["reward_mode"], case["nsub"], case["n"], len(acts)
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    F = mc.data_config.shape[0]
    h = timestep()
    upd = upd_of(rm, nsub)
    kp, kd = golden_gains()
    tab, par = imit_inputs() if rm >= 3 else (None, None)
    r = dict(ctrl=np.zeros((T, n, 28)), obs=np.zeros((T, n, 56)), reward=np.zeros((T, n)), done=np.zeros((T, n), dtype=np.uint8),
             cursor=np.zeros((T + 1, n), dtype=np.int32), cycle=np.zeros((T + 1, n), dtype=np.int32), qpos=np.zeros((n, 35)),
             qacc_warmstart=np.zeros((n, 34)), time=np.zeros(n), peak=np.zeros(n, dtype=np.int32))
    for e in range(n):
        od = O.Data(om); od.reset(); od.set_state(case["q"][e], case["v"][e])
        shadow = O.Data(om); shadow.reset(); shadow.set_state(case["q"][e], case["v"][e])      # the same ctrl, substep by substep: row counts
        cur, init, cyc = int(case["cursor"][e]), int(case["init"][e]), 0
        peak = [int(od.get("nefc", 1)[0])]
        r["cursor"][0, e] = cur
        for t in range(T):
            a = acts[t, e]
            if am in (1, 2):
                k = S.start_frame(rm, cur, init, F, upd)
                c = host_ctrl(am, a, mc.data_config[k], mc.data_vel[k], od.get("qpos", 40), od.get("qvel", 40), kp, kd)
                if rm <= 2:
                    o, rew, dn, cur = od.env_step(c, nsub, rm, mc.data_config, cur, init)
                elif rm == 3:
                    o, rew, dn, cur, cyc = O.env_step_imitation(om, od, c, nsub, tab, par, cur, cyc)
                else:
                    o, rew, dn, cur = O.env_step_v1(om, od, c, nsub, tab, par, float(mc.dt), cur, init)
                shadow.set("ctrl", c)
                for _ in range(nsub):
                    shadow.step(); peak[0] = max(peak[0], int(shadow.get("nefc_peak", 1)[0]))
            else:
                o, rew, dn, nxt, c = S.env_step(cm, od, am, a, mc, cur, nsub, h, reward_mode=rm, frame_init=init, imit=(tab, par), cycle=cyc, peak=peak)
                cur, cyc = nxt if rm == 3 else (nxt, cyc)
            r["ctrl"][t, e] = c; r["obs"][t, e] = o; r["reward"][t, e] = rew; r["done"][t, e] = dn
            r["cursor"][t + 1, e] = cur; r["cycle"][t + 1, e] = cyc
        r["qpos"][e] = od.get("qpos", 40); r["qacc_warmstart"][e] = od.get("qacc_warmstart", 40); r["time"][e] = od.get("time", 1)[0]
        r["peak"][e] = peak[0]
    if key is not None:
        for x in r.values():
            x.setflags(write=False)
        _EXPECTED[key] = r
    return r


def check(case, exp, got, tol=1e-9, envs=None, ws_tol=None):
    """got: dict of what a form produced — ctrl (list of T arrays [n, 28] or None where the form cannot read it between steps), obs, reward, done
    [T, n, .], cursors (list of T arrays or None), init, qpos, qacc_warmstart, time.  Every row of the batch is compared (envs: a subset, for
    callers that compare a subset with something else and the rest here).  -> the worst relative error of ctrl / obs / reward / final qpos."""
    n, T = case["n"], len(exp["obs"])
    envs = range(n) if envs is None else envs
    worst = dict(ctrl=0.0, obs=0.0, reward=0.0, qpos=0.0, qacc_warmstart=0.0)
    for t in range(T):
        for e in envs:
            if got["ctrl"][t] is not None:
                worst["ctrl"] = max(worst["ctrl"], H.rel_err(got["ctrl"][t][e], exp["ctrl"][t, e]))
            worst["obs"] = max(worst["obs"], H.rel_err(got["obs"][t, e], exp["obs"][t, e]))
            worst["reward"] = max(worst["reward"], abs(got["reward"][t, e] - exp["reward"][t, e]) / max(1.0, abs(exp["reward"][t, e])))
            assert bool(got["done"][t, e]) == bool(exp["done"][t, e]), ("done", t, e)
        if got["cursors"][t] is not None:
            assert np.array_equal(np.asarray(got["cursors"][t])[list(envs)], exp["cursor"][t + 1][list(envs)]), ("cursor after step", t, got["cursors"][t], exp["cursor"][t + 1])
    assert np.array_equal(np.asarray(got["init"])[list(envs)], case["init"][list(envs)]), "DM_F_FRAME_INIT moved"
    for e in envs:
        worst["qpos"] = max(worst["qpos"], H.rel_err(got["qpos"][e], exp["qpos"][e]))
        worst["qacc_warmstart"] = max(worst["qacc_warmstart"], H.rel_err(got["qacc_warmstart"][e], exp["qacc_warmstart"][e]))
        assert abs(got["time"][e] - exp["time"][e]) < 1e-12, ("time", e)
    msg = "action mode %d, reward mode %d, %d substeps: %s" % (case["action_mode"], case["reward_mode"], case["nsub"], worst)
    assert worst["ctrl"] < tol and worst["obs"] < tol and worst["reward"] < tol and worst["qpos"] < tol, msg
    assert worst["qacc_warmstart"] < (max(tol, 1e-8) if ws_tol is None else ws_tol), msg
    return worst


def run_steps(b, case, horizon=False):
    """The case through a batch's host-array interface (device or testbench), step by step or as one horizon launch (`b.rollout`: the testbench)."""
    n, T, nsub = case["n"], case["T"], case["nsub"]
    prepare(b, case)
    got = dict(ctrl=[None] * T, cursors=[None] * T)
    if horizon:
        obs, rew, done = b.rollout(case["acts"], nsub)
    else:
        obs = np.zeros((T, n, 56)); rew = np.zeros((T, n)); done = np.zeros((T, n), dtype=np.uint8)
        for t in range(T):
            o, r_, d = b.step(case["acts"][t], nsub)[:3]
            obs[t], rew[t], done[t] = o, r_, d
            got["ctrl"][t] = b.get(A.F_CTRL); got["cursors"][t] = b.get(A.F_FRAME_IDX)
    got["ctrl"][T - 1] = b.get(A.F_CTRL); got["cursors"][T - 1] = b.get(A.F_FRAME_IDX)
    got.update(obs=obs, reward=rew, done=done, init=b.get(A.F_FRAME_INIT), qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL),
               qacc_warmstart=b.get(A.F_QACC_WARMSTART), time=b.get(A.F_TIME))
    return got


def same_bits(x, y, envs=None):
    """two results of run_steps-like dicts, bit for bit, on `envs` (default: all): rows, cursors, final state, the last ctrl"""
    sel = slice(None) if envs is None else list(envs)
    for k in ("obs", "reward", "done"):
        assert np.array_equal(np.asarray(x[k])[:, sel], np.asarray(y[k])[:, sel]), k
    for k in ("init", "qpos", "qvel", "qacc_warmstart", "time"):
        assert np.array_equal(np.asarray(x[k])[sel], np.asarray(y[k])[sel]), k
    assert np.array_equal(x["ctrl"][-1][sel], y["ctrl"][-1][sel]), "ctrl"
    assert np.array_equal(np.asarray(x["cursors"][-1])[sel], np.asarray(y["cursors"][-1])[sel]), "cursor"
