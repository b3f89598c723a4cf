"""Action modes 3 ("spd-target") and 4 ("spd-mocap") — a PD target pose under a stable PD controller evaluated at every simulation substep
(include/dmenv.h DM_OPT_ACTION_MODE) — on the wave testbench: the kernel source of the one-env path (env_step.h spd_control) and of the packed
path (slot_step.h slot_spd_control; DM_OPT_PACKED 1 and 2) against tests/spd_numpy.py, a float64 restatement on the CPU oracle.  The bar is the
project's 1e-9 for HIP == oracle (the restatement's own noise is 3e-13: M + h Kd has a condition number below 100)."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from tests import helpers as H
from tests import spd_numpy as S

TOL = 1e-9
FORMS = [0, 1, 2]          # DM_OPT_PACKED: one env per wave, four per wave, four per wave with the three-set code


def _batch(n, packed, mode, reward_mode=0):
    from tests.emu.emu import EmuBatch
    mc = H.mocap()
    b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, n, 0)
    b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_ACTION_MODE, mode); b.set_option(A.OPT_REWARD_MODE, reward_mode)
    return b


def _start(b, idx, q, v):
    n = len(q)
    b.set(A.F_QACC_WARMSTART, np.zeros((n, 34))); b.set(A.F_TIME, np.zeros(n))
    b.set_state(q, v, frame_idx=idx)


def _oracle_at(om, q, v):
    from oracle import oracle as O
    od = O.Data(om)
    od.reset(); od.set_state(q, v)
    return od


def _timestep(om):
    return float(om.get("timestep")[0])


def _actions(rng, mode, mc, idx, scale):
    """mode 3: target poses around the envs' mocap frames; mode 4: offsets from the frame"""
    off = scale * rng.randn(len(idx), 28)
    return mc.data_config[idx][:, 7:] + off if mode == 3 else off


@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("packed", FORMS)
def test_ctrl_and_state_after_one_step(packed, mode, nsub):
    """DM_F_CTRL is the restatement's last-substep (unclamped) ctrl, and the step's observation / state are those of an oracle step driven with
    the restatement's per-substep ctrls — every env of the batch.  And, independent of how either side solves: with the oracle's M and
    c = qfrc_bias - qfrc_passive at the state the last substep starts from, tau_full = (0_6, gear ctrl) and a = M^-1 (tau_full - c), the
    kernel's ctrl satisfies the rule  tau = kp (qbar - q - h v) + kd (vbar - v - h a)  on the hinge dofs."""
    n = 8
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    h = _timestep(om)
    idx, q, v, _ws, _c = H.varied_states(n, seed=3)
    act = _actions(np.random.RandomState(10 * mode + nsub), mode, mc, idx, 0.3)
    b = _batch(n, packed, mode)
    _start(b, idx, q, v)
    obs, _rew, done = b.step(act, nsub)
    kctrl = b.get(A.F_CTRL); kq = b.get(A.F_QPOS); kv = b.get(A.F_QVEL)
    kp, kd = S.gains(cm)
    gear = cm.actuator_gear
    worst = dict(ctrl=0.0, obs=0.0, state=0.0, identity=0.0)
    for e in range(n):
        od = _oracle_at(om, q[e], v[e])
        qbar, vbar = S.targets(mode, act[e], mc, int(idx[e]))
        for _ in range(nsub - 1):
            S.substep(cm, od, qbar, vbar, h)
        M, c, q0, v0 = S.smooth_terms(od)              # the state the last substep starts from
        ctrl = S.substep(cm, od, qbar, vbar, h)
        worst["ctrl"] = max(worst["ctrl"], H.rel_err(kctrl[e], ctrl))
        worst["obs"] = max(worst["obs"], H.rel_err(obs[e], od.obs()))
        worst["state"] = max(worst["state"], H.rel_err(kq[e], od.get("qpos")), H.rel_err(kv[e], od.get("qvel")))
        assert bool(done[e]) == od.is_done()
        tau_full = np.zeros(34); tau_full[6:] = gear * kctrl[e]
        a = np.linalg.solve(M, tau_full - c)
        tau = kp[6:] * (qbar - q0[7:] - h * v0[6:]) + kd[6:] * (vbar - v0[6:] - h * a[6:])
        worst["identity"] = max(worst["identity"], H.rel_err(tau_full[6:], tau))
    print("packed %d mode %d nsub %d: worst rel err %s" % (packed, mode, nsub, worst))
    for k, w in worst.items():
        assert w < TOL, "%s: rel err %.3e" % (k, w)
    assert np.abs(kctrl).max() > 0.5, "the states must drive some actuators past their ctrlrange (the stored ctrl is the unclamped one)"


@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("packed", FORMS)
def test_lockstep_rollout_matches_the_restatement(packed, mode, nsub):
    """15 steps of 6 envs (the size of test_rollout_matches_oracle_on_testbench) in lock step with the restatement, reward mode 1 so that the
    frame cursor — which mode 4 reads — moves; auto-reset off.  obs, reward, done and the cursor every step, final qpos / qacc_warmstart / time,
    at the bars of helpers.compare_rollout."""
    n, steps = 6, 15
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    h = _timestep(om)
    idx, q, v, _ws, _c = H.varied_states(n, seed=5)
    b = _batch(n, packed, mode, reward_mode=1)
    _start(b, idx, q, v)
    ods = [_oracle_at(om, q[e], v[e]) for e in range(n)]
    fidx = idx.astype(np.int64).copy()
    rng = np.random.RandomState(1)
    worst = 0.0
    for t in range(steps):
        act = _actions(rng, mode, mc, fidx, 0.2)
        obs, rew, done = b.step(act, nsub)
        for e in range(n):
            o, r, d, nxt, _c2 = S.env_step(cm, ods[e], mode, act[e], mc, int(fidx[e]), nsub, h, reward_mode=1)
            fidx[e] = nxt
            worst = max(worst, H.rel_err(obs[e], o), abs(rew[e] - r) / max(1.0, abs(r)))
            assert bool(done[e]) == d, (t, e)
        assert np.array_equal(b.get(A.F_FRAME_IDX), fidx.astype(np.int32))
    print("packed %d mode %d nsub %d: rollout worst rel err %.3e" % (packed, mode, nsub, worst))
    assert worst < TOL, "rollout rel err %.3e" % worst
    qf = b.get(A.F_QPOS); wf = b.get(A.F_QACC_WARMSTART); tf = b.get(A.F_TIME)
    for e in range(n):
        assert H.rel_err(qf[e], ods[e].get("qpos")) < TOL
        assert H.rel_err(wf[e], ods[e].get("qacc_warmstart")) < max(TOL, 1e-8)
        assert abs(tf[e] - ods[e].get("time")[0]) < 1e-12


@pytest.mark.parametrize("packed", [0, 1])
def test_two_substeps_differ_from_a_held_torque(packed):
    """The control is evaluated at the start of EVERY substep: one env step of two substeps must not equal a step whose first-substep ctrl is
    held through both (what modes 1 and 2 do).  40 walk frames, targets 0.1 rad off the frame: the restatement alone gives
    max |dqpos| = 2.5e-3 .. 7.6e-3 between the two, so 1e-4 leaves a factor of 25."""
    n = 40
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    h = _timestep(om)
    F = mc.data_config.shape[0]
    idx = (np.arange(n) * F // n).astype(np.int32)
    q = mc.data_config[idx].copy(); v = mc.data_vel[idx].copy()
    act = q[:, 7:] + 0.1
    b = _batch(n, packed, 3)
    _start(b, idx, q, v)
    b.step(act, 2)
    kq = b.get(A.F_QPOS)
    diffs = []
    for e in range(n):
        od = _oracle_at(om, q[e], v[e])
        od.set("ctrl", S.spd_ctrl(cm, od, act[e], np.zeros(28), h))
        od.step(); od.step()
        diffs.append(float(np.abs(kq[e] - od.get("qpos")).max()))
    print("packed %d: max |dqpos| against a held first-substep ctrl: %.2e .. %.2e" % (packed, min(diffs), max(diffs)))
    assert min(diffs) > 1e-4


@pytest.mark.parametrize("mode", [3, 4])
def test_redo_path_applies_the_same_control(mode):
    """Packed envs that exceed a capacity of the packed path are re-stepped by the one-env code, which must apply the same rule: the same
    inputs through the one-env path give the same results (the bar of the packed-against-one-env tests, 1e-11)."""
    cm, mc = H.compiled_model(), H.mocap()
    hi, hq, hv = H.many_row_states(40, 64, want=4)
    li, lq, lv, _ws, _c = H.varied_states(4, seed=9)
    idx = np.concatenate([hi, li]).astype(np.int32); q = np.concatenate([hq, lq]); v = np.concatenate([hv, lv])
    n = len(q)
    act = _actions(np.random.RandomState(4), mode, mc, idx, 0.2)
    outs = []
    for packed in (1, 0):
        b = _batch(n, packed, mode)
        _start(b, idx, q, v)
        obs, _rew, done = b.step(act, 2)
        outs.append((obs, done, b.get(A.F_QPOS), b.get(A.F_QVEL), b.get(A.F_QACC_WARMSTART), b.get(A.F_CTRL), b.redo_total()))
    assert outs[0][-1] >= len(hq) and outs[1][-1] == 0, "the many-row states must leave the packed path (%d re-stepped)" % outs[0][-1]
    for x, y in zip(outs[0][:-1], outs[1][:-1]):
        assert H.rel_err(x, y) < 1e-11
    for x, y in zip(outs[0][:-1], outs[1][:-1]):          # the re-stepped envs ran the one-env code on the same inputs: the same bits
        assert np.array_equal(x[:len(hq)], y[:len(hq)])


def test_parked_kinematics_feed_the_controller_unchanged():
    """With the imitation reward the one-env step parks the kinematics of the state it leaves (env_step.h save_kin) and the next step starts from
    them: in modes 3 and 4 the controller's pass is their first consumer.  Same bits as a run whose parked kinematics are dropped before every step."""
    from deepmimic_mujoco_amd.imitation import ImitationSpec
    from tests.emu.emu import EmuBatch
    mc = H.mocap()
    n, T = 4, 3
    imit = ImitationSpec(H.compiled_model()).table_for(mc)
    idx, q, v, _ws, _c = H.varied_states(n, seed=12)
    idx[:] = np.minimum(idx, mc.data_config.shape[0] - T - 2)
    act = _actions(np.random.RandomState(6), 4, mc, idx, 0.1)
    outs = []
    for drop in (False, True):
        b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, n, 0, imitation=imit)
        b.set_option(A.OPT_ACTION_MODE, 4); b.set_option(A.OPT_REWARD_MODE, 3)
        _start(b, idx, q, v)
        rows = []
        for _t in range(T):
            if drop:
                b.set(A.F_QPOS, b.get(A.F_QPOS))          # (a field write invalidates the parked kinematics)
            obs, rew, done = b.step(act, 2)
            rows.append((obs.copy(), rew.copy(), done.copy(), b.get(A.F_CTRL)))
        outs.append(rows)
    for x, y in zip(*outs):
        for a_, b_ in zip(x, y):
            assert np.array_equal(a_, b_)
    assert np.isfinite(outs[0][-1][0]).all()
