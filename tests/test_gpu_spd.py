"""Action modes 3 ("spd-target") and 4 ("spd-mocap") through the C ABI on the device: every launch form that can step a batch against
tests/spd_numpy.py (a float64 restatement of the stable PD rule on the CPU oracle), the fall-backs of dm_batch_rollout and DM_OPT_STEP_QUEUE,
the option range, the float32 library and a full-size DPVecEnv run.  tests/test_spd.py checks the same kernel source on the wave testbench."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch, DPVecEnv
from tests import helpers as H
from tests import spd_numpy as S
from tests import gpu_batch as GB
from tests.gpu_batch import DEV, horizon_rows, start, step_rows

pytestmark = pytest.mark.gpu
TOL = 1e-9

# the launch forms of tests/gpu_batch.py that step in these modes (the *_spd kernels; dm_batch_rollout issues step launches)
FORMS = {k: GB.FORMS[k] for k in ("narrow", "packed", "packed-ext", "narrow-act", "packed-act", "rollout", "rollout-act", "rollout-narrow-act")}


def _make(n, mode, packed, reward_mode=1, dtype=64):
    mc = H.mocap()
    b = Batch(H.compiled_model(), mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt), dtype=dtype)
    b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_ACTION_MODE, mode); b.set_option(A.OPT_REWARD_MODE, reward_mode)
    return b


def _run(form, mode, nsub, idx, q, v, T, first_action, want_ctrl=True):
    """T steps of the batch through one launch form.  Returns the rows (actions [T, n, 28] as consumed, obs, rew, done), the per-step
    DM_F_CTRL where the form allows reading it between steps (else only the last), and the final state."""
    lf = FORMS[form]
    n = len(q)
    b = _make(n, mode, lf.packed)
    start(b, idx, q, v)
    ac, ob, rew, dn, vp = horizon_rows(T, n, act=first_action)   # open loop: every row given; with a policy rows 1.. are overwritten
    pol, W = GB.fused_policy() if lf.policy else (None, None)
    ctrls = []
    GB.issue_steps(b, lf, ac, ob, rew, dn, nsub, pol=pol, W=W, vp=vp, between=(lambda t: ctrls.append(b.get(A.F_CTRL))) if want_ctrl else None)
    if not ctrls:
        ctrls = [None] * (T - 1) + [b.get(A.F_CTRL)]
    final = (b.get(A.F_QPOS), b.get(A.F_QVEL), b.get(A.F_QACC_WARMSTART), b.get(A.F_TIME), b.get(A.F_FRAME_IDX), b.get(A.F_CTRL))
    stats = (b.queue_stats(), b.redo_total())
    b.close()
    return (ac.cpu().numpy(), ob.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy()), ctrls, final, stats


def _first_action(mode, idx, seed, n_rows):
    """[T + 1, n, 28]: mode 3 target poses around the envs' starting frames, mode 4 offsets"""
    mc = H.mocap()
    off = 0.2 * np.random.RandomState(seed).randn(n_rows, len(idx), 28)
    return mc.data_config[idx][None, :, 7:] + off if mode == 3 else off


@pytest.mark.parametrize("nsub", [1, 2])
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_launch_forms_match_the_restatement(form, mode, nsub):
    """Lock step with the restatement (reward mode 1: the frame cursor that mode 4 reads moves; auto-reset off): DM_F_CTRL — the last
    substep's unclamped ctrl — after every step the form lets us read it, obs / reward / done every step, the final qpos /
    qacc_warmstart / time and the cursor, at the bars of helpers.compare_rollout.  13 envs: a last packed wave with spare slots."""
    from oracle import oracle as O
    n, T = 13, 15
    cm, mc, om = H.compiled_model(), H.mocap(), H.oracle_model()
    h = float(om.get("timestep")[0])
    idx, q, v, _ws, _c = H.varied_states(n, seed=5)
    rows, ctrls, final, _stats = _run(form, mode, nsub, idx, q, v, T, _first_action(mode, idx, 1, T + 1))
    ac, ob, rew, dn = rows
    ods = []
    for e in range(n):
        od = O.Data(om); od.reset(); od.set_state(q[e], v[e]); ods.append(od)
    fidx = idx.astype(np.int64).copy()
    worst, worst_ctrl = 0.0, 0.0
    for t in range(T):
        for e in range(n):
            o, r, d, nxt, c = S.env_step(cm, ods[e], mode, ac[t, e], mc, int(fidx[e]), nsub, h, reward_mode=1)
            fidx[e] = nxt
            worst = max(worst, H.rel_err(ob[t, e], o), abs(rew[t, e] - r) / max(1.0, abs(r)))
            assert bool(dn[t, e]) == d, (t, e)
            if ctrls[t] is not None:
                worst_ctrl = max(worst_ctrl, H.rel_err(ctrls[t][e], c))
    print("%s mode %d nsub %d: worst rel err obs / reward %.3e, ctrl %.3e" % (form, mode, nsub, worst, worst_ctrl))
    assert worst < TOL and worst_ctrl < TOL
    qf, _vf, wf, tf, ff, _cf = final
    assert np.array_equal(ff, fidx.astype(np.int32))
    for e in range(n):
        assert H.rel_err(qf[e], ods[e].get("qpos")) < TOL
        assert H.rel_err(wf[e], ods[e].get("qacc_warmstart")) < max(TOL, 1e-8)
        assert abs(tf[e] - ods[e].get("time")[0]) < 1e-12


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("pair", [("rollout", "packed"), ("rollout-act", "packed-act"), ("rollout-narrow-act", "narrow-act")])
def test_rollout_falls_back_to_step_launches_bit_for_bit(pair, mode):
    """dm_batch_rollout in modes 3 and 4 issues per-step launches: every row and the final state are those of T dm_batch_step /
    dm_batch_step_act calls, bit for bit (two many-row states make the packed launches hand envs to the redo kernel)."""
    n, T = 37, 12
    idx, q, v, _ws, _c = H.varied_states(n, seed=8)
    hi, hq, hv = H.many_row_states(40, 64, want=2)
    for e, k in ((1, 0), (n - 3, -1)):
        q[e], v[e], idx[e] = hq[k], hv[k], hi[k]
    fa = _first_action(mode, idx, 3, T + 1)
    x = _run(pair[0], mode, 2, idx, q, v, T, fa, want_ctrl=False)
    y = _run(pair[1], mode, 2, idx, q, v, T, fa, want_ctrl=False)
    for i in range(4):
        assert np.array_equal(x[0][i], y[0][i]), "row arrays differ (%d)" % i
    for i in range(6):
        assert np.array_equal(x[2][i], y[2][i]), "final state differs (%d)" % i
    assert np.isfinite(x[0][1]).all()
    if FORMS[pair[0]].packed:
        assert x[3][1] == y[3][1] > 0, "the many-row states must go through the redo kernel (%d / %d)" % (x[3][1], y[3][1])


@pytest.mark.parametrize("mode", [3, 4])
def test_step_queue_launches_every_call_at_once(mode):
    """A batch with DM_OPT_STEP_QUEUE set steps exactly like one without in modes 3 and 4, and nothing is ever queued."""
    n, T = 256, 10
    outs = []
    for queue in (0, 8):
        env = DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=3, packed=True, frame_skip=1,
                       action_mode="spd-target" if mode == 3 else "spd-mocap", step_queue=queue)
        b = env.batch
        g = torch.Generator(device=DEV); g.manual_seed(11)
        ac = torch.randn((T, n, 28), generator=g, dtype=torch.float64, device=DEV) * 0.3
        _ac, ob, rew, dn, _vp = horizon_rows(T, n)
        env.reset("rsi")
        for t in range(T):
            b.step(ac[t], 1, (ob[t], rew[t], dn[t]))
            if queue:
                assert b.queue_stats() == (0, 0, 0)
        b.join(); b.sync()
        assert b.queue_stats() == (0, 0, 0)
        outs.append((ob.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy(), b.get(A.F_QPOS), b.get(A.F_QVEL), b.get(A.F_QACC_WARMSTART),
                     b.get(A.F_FRAME_IDX), b.get(A.F_EPISODE), b.get(A.F_CTRL)))
        env.close()
    for i, (x, y) in enumerate(zip(*outs)):
        assert np.array_equal(x, y), "queue on / off differ (%d)" % i
    assert np.isfinite(outs[0][0]).all()


def test_action_mode_option_range():
    b = _make(4, 0, 0, reward_mode=0)
    for m in (3, 4, 0):
        b.set_option(A.OPT_ACTION_MODE, m)
    for bad in (5, -1):
        with pytest.raises(A.DmenvError, match="action mode"):
            b.set_option(A.OPT_ACTION_MODE, bad)
    b.close()


def test_float32_library_tracks_the_float64_path_in_mode_3():
    """libdmenv32.so is a tracking path, not a parity path (test_float32_batch_tracks_the_float64_path): one step from identical states, float32
    against float64, over the envs whose row counts agree (their share above that test's 0.9); reproducible and finite.  The yardstick for the
    error is action mode 2 — existing code — on the same states and the same action array: mode 3's median relative obs error may be at most
    4x mode 2's (one more float32 solve with cond <= 92 adds ~cond * eps = 1e-5 on `a`, which enters tau scaled by h kd <= 1.66 — the size of
    mode 2's own kp eps |q| term — with a factor for the two further roundings).
    The same ratio holds mode 4 ("spd-mocap", the stable form of mode 2: the same solve on top of the same mocap rows) to mode 2 under reward
    mode 2, where both look their frame up as (cursor + init) % F: the cursors are written past the clip's 39 frames for most envs."""
    mc = H.mocap()
    n = 256
    idx, q, v, _ws, _c = H.varied_states(n, seed=31)
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    a = np.random.RandomState(2).randn(n, 28) * 0.5
    cursor = (7 * np.arange(n, dtype=np.int32)) % 90
    assert (cursor >= mc.data_config.shape[0]).mean() > 0.5
    for reward_mode, modes in ((0, (2, 3)), (2, (2, 4))):
        med = {}
        for mode in modes:
            outs = {}
            for dt in (64, 32, 32):
                b = _make(n, mode, 0, reward_mode=reward_mode, dtype=dt)
                start(b, idx, q, v)
                if reward_mode == 2:
                    b.set(A.F_FRAME_IDX, cursor)
                nefc0 = b.get(A.F_NEFC).copy()
                obs, _rew, done = b.step(a)
                outs.setdefault(dt, []).append((obs.copy(), done.copy(), nefc0, b.get(A.F_NEFC).copy(), b.get(A.F_QPOS).copy()))
                b.close()
            o64, _d64, n64a, n64b, _q64 = outs[64][0]
            o32, _d32, n32a, n32b, q32 = outs[32][0]
            assert np.array_equal(o32, outs[32][1][0]) and np.array_equal(q32, outs[32][1][4])          # reproducible
            assert np.isfinite(o32).all()
            same = (n64a == n32a) & (n64b == n32b)
            assert same.mean() > 0.9, (mode, same.mean())
            err = np.abs(o32 - o64).max(1) / np.maximum(1.0, np.abs(o64).max(1))
            med[mode] = float(np.median(err[same]))
        m = modes[1]
        print("float32 vs float64 after one step, reward mode %d, median rel obs err: mode 2 (pd) %.3e, mode %d %.3e, ratio %.2f" % (reward_mode, med[2], m, med[m], med[m] / med[2]))
        assert med[m] <= 4 * med[2]


def test_dpvecenv_spd_mocap_full_size_open_loop():
    """DPVecEnv(action_mode="spd-mocap") at 4 096 envs, imitation reward, frame_skip='mocap', 64 steps of zero action (tracking the clip open loop):
    every observation finite, no environment ever flags a solver problem (DM_F_STATUS bit 1).  Balance is NOT asserted: open-loop tracking falls
    after 23-44 frames on `walk` with either controller — that is what the policy is for."""
    n = 4096
    env = DPVecEnv(n, motion="walk", device=0, reward="imitation", autoreset="rsi", seed=1, frame_skip="mocap", action_mode="spd-mocap")
    assert env.frame_skip >= 2
    b = env.batch
    zero = torch.zeros((n, 28), dtype=torch.float64, device=DEV)
    out = step_rows(n)
    env.reset("rsi")
    ndone, rsum = 0, 0.0
    for t in range(64):
        b.step(zero, env.frame_skip, out)
        b.join()
        assert bool(torch.isfinite(out[0]).all()), t
        assert int((b.get(A.F_STATUS) & 2).sum()) == 0, t
        ndone += int(out[2].sum()); rsum += float(out[1].mean())
    print("spd-mocap, %d envs x 64 steps x %d substeps, zero action: mean reward %.3f, %d episodes ended, dm_batch_redo_total %d (packed: %s)"
          % (n, env.frame_skip, rsum / 64, ndone, b.redo_total(), env.packed))
    env.close()


def test_spd_target_action_space_is_the_joint_range():
    env = DPVecEnv(8, motion="walk", device=0, action_mode="spd-target")
    cm = H.compiled_model()
    jr = cm.jnt_range[cm.actuator_jntid]
    assert np.allclose(env.action_space.low, jr[:, 0]) and np.allclose(env.action_space.high, jr[:, 1])
    assert env.batch.options[A.OPT_ACTION_MODE] == A.ACTION_SPD_TARGET
    env.close()
    with pytest.raises(ValueError):
        DPVecEnv(8, motion="walk", device=0, action_mode="spd")
