"""dm_batch_state_features on the GPU (csrc/state_kernel.h): DeepMimic's state features against the float64 restatement
(tests/state_numpy.py) for explicit states and for the batch's own state, the `obs_mode="deepmimic"` facades, repeatability, argument
checks, the segment collector and training through the tools at width 171.

Bars.  float64 library: the project's 1e-9, compared as tests/test_gpu_spd.py compares (largest absolute difference over
max(1, largest reference magnitude)).  float32 library: phase, height and the pose block 1e-5 absolute (the bar
test_geom_xform_matches_kinematics uses for float32 kinematics); the velocity block 1e-5 max(1, |qvel|_1) per state — each component
is a sum over at most 34 dofs of |qvel_i| times a lever arm of about a metre.  A quaternion whose reference |w| is below 1e-6 may
match up to sign (the sign rule is discontinuous at w = 0); at most 0.1 % of the (state, body) pairs may be compared that way.
Worst observed on an MI355X: float64 1.1e-15 (explicit states) and 2.2e-15 (batch state, facades, auto-reset rows); float32 2.7e-7 on
the pose block and 0.7 % of the velocity bar; no pair compared up to sign."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch, DPEnv, DPVecEnv, MlpPolicy
from deepmimic_mujoco_amd.dp_env import REWARD_MODES
from tests import helpers as H
from tests import state_numpy as SN
from tests.test_state_features import bar_states

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL64, TOL32 = 1e-9, 1e-5
MODE_NAMES = {v: k for k, v in REWARD_MODES.items()}


def batch(n, dtype=64, clip="walk"):
    mc = H.mocap(clip)
    return Batch(H.compiled_model(), mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt), dtype=dtype)


def check(got, ref, qvel, dtype, what):
    """the bars of this file's docstring; prints the worst errors before it asserts"""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape == (len(qvel), SN.NSTATE)
    if dtype == 64:
        fails, e_pose, e_vel, loose = SN.compare(got, ref, np.inf, np.inf)          # (aligns the signs, counts the pairs)
        aligned = got.copy()
        for i in range(len(ref)):
            for k in range(SN.NBODY):
                c = SN.QUAT_IDX[k]
                if abs(ref[i, c[0]]) < SN.W_SMALL and np.abs(got[i, c] + ref[i, c]).max() < np.abs(got[i, c] - ref[i, c]).max():
                    aligned[i, c] = -got[i, c]
        worst = max(H.rel_err(aligned[i], ref[i]) for i in range(len(ref)))
        print("%s float64: worst relative error %.3e (pose block %.3e absolute), %d pairs up to sign" % (what, worst, e_pose, loose))
        assert loose <= 1e-3 * len(ref) * SN.NBODY
        assert worst < TOL64, worst
        return worst
    bar = TOL32 * np.maximum(1.0, np.abs(np.asarray(qvel)).sum(1))
    fails, e_pose, e_vel, loose = SN.compare(got, ref, TOL32, bar)
    print("%s float32: worst pose-block error %.3e (bar %.0e), worst velocity error %.3f of its bar, %d pairs up to sign" % (what, e_pose, TOL32, e_vel, loose))
    assert loose <= 1e-3 * len(ref) * SN.NBODY
    assert not fails, fails[:10]
    return e_pose, e_vel


def fields_reference(b, mode, ids=None):
    """the restatement of the batch's fields as they are now -> (features [n,171], qvel [n,34])"""
    cm = H.compiled_model()
    q, v = b.get(A.F_QPOS), b.get(A.F_QVEL)
    fi, fin = b.get(A.F_FRAME_IDX), b.get(A.F_FRAME_INIT)
    ids = np.arange(b.n) if ids is None else np.asarray(ids)
    ph = [SN.phase_of(mode, fi[e], fin[e], b.n_frames) for e in ids]
    return SN.batch_features(cm, q[ids], v[ids], ph), v[ids]


# ---- explicit states ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_explicit_states_match_the_restatement(dtype):
    cm = H.compiled_model()
    q, v, phase = bar_states()
    ref = SN.batch_features(cm, q, v, phase)
    b = batch(4, dtype)
    got = b.state_features(qpos=q, qvel=v, phase=phase)
    check(got, ref, v, dtype, "explicit states (%d)" % len(q))
    tq, tv, tp = (torch.as_tensor(x, device=DEV) for x in (q, v, phase))
    out = torch.zeros((len(q), A.NSTATE), dtype=torch.float64, device=DEV)
    assert b.state_features(out=out, qpos=tq, qvel=tv, phase=tp) is out
    np.testing.assert_array_equal(out.cpu().numpy(), got)                      # host and device pointers: the same launch
    # far from the world origin the features are the same (the kernel drops the root's x and y)
    q2 = q.copy(); q2[:, 0] += 250.0; q2[:, 1] -= 80.0
    np.testing.assert_array_equal(b.state_features(qpos=q2, qvel=v, phase=phase), got)
    b.close()


# ---- the batch's own state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype,packed", [(64, False), (64, True), (32, False)])
def test_batch_state_rows(dtype, packed, mode):
    n = 48
    env = DPVecEnv(n, motion="walk", reward=MODE_NAMES[mode], autoreset="rsi", seed=3, dtype=dtype, packed=packed)
    b = env.batch
    assert env.packed or not packed
    idx, q, v, _ws, _ctrl = H.varied_states(n, seed=11 + mode)
    b.set_state(q, v, frame_idx=idx)
    b.set(A.F_FRAME_INIT, ((idx * 7 + 3) % b.n_frames).astype(np.int32))
    ref, qv = fields_reference(b, mode)
    check(b.state_features(), ref, qv, dtype, "after set_state, mode %d" % mode)
    ids = np.array([5, 0, 47, 5, 13], dtype=np.int32)
    sub = b.state_features(env_ids=ids)
    check(sub, ref[ids], qv[ids], dtype, "env_ids subset")
    np.testing.assert_array_equal(b.state_features(env_ids=torch.as_tensor(ids, device=DEV)).cpu().numpy(), sub)
    env.reset("rsi")
    rng = np.random.RandomState(mode)
    dones = 0
    for t in range(12):
        _o, _r, d, _i = env.step(rng.randn(n, 28) * 0.9)
        dones += int(np.asarray(d).sum())
        if t % 4 == 3:
            ref, qv = fields_reference(b, mode)
            check(b.state_features(), ref, qv, dtype, "after step %d, mode %d" % (t + 1, mode))
    head = b.state_features(env_ids=np.arange(7, dtype=np.int32))
    np.testing.assert_array_equal(head, b.state_features()[:7])
    env.close()


# ---- the facades ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_buffers", [False, True])
def test_dpvecenv_deepmimic_observation(device_buffers):
    n, steps = 32, 80
    kw = dict(motion="walk", reward="imitation", autoreset="rsi", seed=5)
    env = DPVecEnv(n, obs_mode="deepmimic", **kw)
    base = DPVecEnv(n, **kw)
    assert env.observation_space.shape == (171,) and base.observation_space.shape == (56,)
    conv = (lambda x: torch.as_tensor(x, device=DEV)) if device_buffers else (lambda x: x)
    host = lambda x: x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    ob = env.reset("rsi"); base.reset("rsi")
    ref, qv = fields_reference(env.batch, 3)
    check(host(ob), ref, qv, 64, "reset")
    rng = np.random.RandomState(1)
    finished, worst = 0, 0.0
    for t in range(steps):
        a = rng.randn(n, 28) * 1.5
        ob, rew, done, _ = env.step(conv(a))
        _ob0, rew0, done0, _ = base.step(conv(a))
        assert host(ob).shape == (n, 171)
        np.testing.assert_array_equal(host(rew), host(rew0)); np.testing.assert_array_equal(host(done), host(done0))
        for f in (A.F_QPOS, A.F_QVEL, A.F_FRAME_IDX, A.F_EPISODE):
            np.testing.assert_array_equal(env.batch.get(f), base.batch.get(f))
        finished += int(host(done).sum())
        ref, qv = fields_reference(env.batch, 3)                      # every step, the rows reset in it included (the fresh episode's state)
        worst = max(worst, check(host(ob), ref, qv, 64, "step %d (%d done)" % (t, int(host(done).sum()))))
    assert finished >= 3, "no environment finished: the auto-reset rows were not covered"
    # the caller's buffers
    if device_buffers:
        out = (torch.zeros((n, 171), dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV))
    else:
        out = (np.zeros((n, 171)), np.zeros(n), np.zeros(n, dtype=np.uint8))
    a = rng.randn(n, 28)
    r = env.step(conv(a), out=out)
    assert r[0] is out[0]
    ref, qv = fields_reference(env.batch, 3)
    check(host(out[0]), ref, qv, 64, "step into the caller's buffers")
    env.close(); base.close()
    with pytest.raises(ValueError):
        DPVecEnv(4, obs_mode="deep-mimic")


def test_dpenv_deepmimic_observation():
    random.seed(4)
    env = DPEnv(motion="walk", reward="v3-config", obs_mode="deepmimic")
    random.seed(4)
    base = DPEnv(motion="walk", reward="v3-config")
    assert env.observation_space.shape == (171,) and base.observation_space.shape == (56,)
    for e in (env, base):
        random.seed(9); e.seed(2)
        e._first = e.reset()
    assert env._first.shape == (171,) and base._first.shape == (56,)
    ref, qv = fields_reference(env._batch, 1)
    check(env._first[None], ref, qv, 64, "DPEnv.reset")
    assert ref[0, SN.O_PHASE] == env.idx_init / float(env.mocap_data_len)
    rng = np.random.RandomState(0)
    for t in range(10):
        a = rng.randn(28) * 0.5
        ob, rew, done, _ = env.step(a)
        ob0, rew0, done0, _ = base.step(a)
        assert rew == rew0 and done == done0 and env.idx_curr == base.idx_curr
        np.testing.assert_array_equal(env.sim.data.qpos, base.sim.data.qpos); np.testing.assert_array_equal(env.sim.data.qvel, base.sim.data.qvel)
        ref, qv = fields_reference(env._batch, 1)
        check(ob[None], ref, qv, 64, "DPEnv.step %d" % t)
    ob = env.reset_model_init()
    ref, qv = fields_reference(env._batch, 1)
    check(ob[None], ref, qv, 64, "DPEnv.reset_model_init")
    env.close(); base.close()
    with pytest.raises(ValueError):
        DPEnv(motion="walk", obs_mode="nope")


def test_dpenv_alive_phase_is_the_rsi_draw():
    random.seed(6)
    env = DPEnv(motion="walk", obs_mode="deepmimic")                  # reward "alive": the cursor never advances
    random.seed(6)
    base = DPEnv(motion="walk")
    for e in (env, base):
        random.seed(12); e.seed(3)
        e._first = e.reset()
    n = float(env.mocap_data_len)
    assert env.idx_init == base.idx_init and env._first[SN.O_PHASE] == env.idx_init / n
    rng = np.random.RandomState(2)
    for t in range(6):
        a = rng.randn(28) * 0.5
        ob, rew, done, _ = env.step(a)
        _ob0, rew0, done0, _ = base.step(a)
        assert rew == rew0 and done == done0 and ob[SN.O_PHASE] == env.idx_init / n
        np.testing.assert_array_equal(env.sim.data.qpos, base.sim.data.qpos); np.testing.assert_array_equal(env.sim.data.qvel, base.sim.data.qvel)
        ref, qv = fields_reference(env._batch, 0)
        check(ob[None], ref, qv, 64, "DPEnv alive step %d" % t)
    env.close(); base.close()


# ---- repeatability, read-only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_two_calls_are_bit_identical_and_change_nothing(dtype):
    n = 40
    b = batch(n, dtype, "spinkick")
    b.set_option(A.OPT_REWARD_MODE, 1)
    idx, q, v, ws, _ctrl = H.varied_states(n, seed=2, clip="spinkick")
    b.set_state(q, v, frame_idx=idx)
    b.step(np.random.RandomState(0).randn(n, 28))
    fields = (A.F_QPOS, A.F_QVEL, A.F_QACC_WARMSTART, A.F_TIME, A.F_FRAME_IDX, A.F_FRAME_INIT, A.F_XIPOS, A.F_CTRL, A.F_EPISODE, A.F_CYCLE, A.F_NEFC)
    before = [b.get(f).copy() for f in fields]
    one = b.state_features()
    two = b.state_features()
    np.testing.assert_array_equal(one, two)
    dev = b.state_features(out=torch.zeros((n, A.NSTATE), dtype=torch.float64, device=DEV))
    np.testing.assert_array_equal(dev.cpu().numpy(), one)
    for f, x in zip(fields, before):
        np.testing.assert_array_equal(b.get(f), x)
    b.close()


# ---- argument errors --------------------------------------------------------------------------------------------------------------------
def test_argument_errors():
    n = 8
    b = batch(n)
    L = b._L
    out = np.zeros((2 * n, A.NSTATE)); q = np.zeros((n, A.NQ)); v = np.zeros((n, A.NV)); ph = np.zeros(n)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def err(rc, word):
        assert rc == -1                                                   # DM_EINVAL
        assert word in L.dm_last_error().decode(), L.dm_last_error()
    err(L.dm_batch_state_features(b._h, None, None, None, None, n + 1, p(out), A.PTR_HOST), "exceeds the batch")
    err(L.dm_batch_state_features(b._h, None, None, None, None, 0, p(out), A.PTR_HOST), "positive")
    err(L.dm_batch_state_features(b._h, p(q), p(v), None, None, n, p(out), A.PTR_HOST), "needs qpos, qvel and phase")
    err(L.dm_batch_state_features(b._h, p(q), None, p(ph), None, n, p(out), A.PTR_HOST), "needs qpos, qvel and phase")
    err(L.dm_batch_state_features(b._h, None, p(v), None, None, n, p(out), A.PTR_HOST), "needs qpos, qvel and phase")
    err(L.dm_batch_state_features(b._h, None, None, None, None, n, p(out), 7), "ptr_kind")
    err(L.dm_batch_state_features(b._h, None, None, None, None, n, None, A.PTR_HOST), "null")
    ids = np.array([0, n], dtype=np.int32)
    err(L.dm_batch_state_features(b._h, None, None, None, p(ids), 2, p(out), A.PTR_HOST), "out of range")
    err(L.dm_batch_state_features(b._h, p(q), p(v), p(ph), p(ids), 2, p(out), A.PTR_HOST), "env_ids must be NULL")
    with pytest.raises(ValueError):
        b.state_features(qpos=q, qvel=v)
    with pytest.raises(ValueError):
        b.state_features(qpos=q, qvel=v, phase=ph, env_ids=ids)
    assert b.state_features(qpos=cm_rest(n), qvel=v, phase=ph).shape == (n, A.NSTATE)         # explicit states may exceed nothing: n is theirs
    assert b.state_features(qpos=np.tile(cm_rest(1), (3 * n, 1)), qvel=np.zeros((3 * n, A.NV)), phase=np.zeros(3 * n)).shape == (3 * n, A.NSTATE)
    b.close()


def cm_rest(n):
    return np.tile(H.compiled_model().qpos0, (n, 1))


# ---- the segment collector ----------------------------------------------------------------------------------------------------------------
def test_segment_collector_on_a_deepmimic_env():
    from deepmimic_mujoco_amd.rollout import RolloutBlock, SegmentCollector
    n, T = 64, 16
    kw = dict(motion="walk", reward="imitation", autoreset="rsi", seed=8, obs_mode="deepmimic")
    env = DPVecEnv(n, **kw)
    pi = MlpPolicy(ob_dim=171, device=DEV, seed=1); pi.seed(1)
    c = SegmentCollector(pi, env, T, stochastic=True, fused=False, first_reset="rsi")
    c.launch()
    ac64 = c.ac64[:T].clone()
    seg = c.collect()
    assert seg["ob"].shape == (T, n, 171) and seg["ob"].dtype == torch.float32
    twin = DPVecEnv(n, **kw)
    ob = torch.zeros((n, 171), dtype=torch.float64, device=DEV)
    twin.reset("rsi", out=ob)
    for t in range(T):
        np.testing.assert_array_equal(seg["ob"][t].cpu().numpy(), ob.to(torch.float32).cpu().numpy())
        ob, rew, done, _ = twin.step(ac64[t])
        np.testing.assert_array_equal(seg["rew"][t].cpu().numpy(), rew.to(torch.float32).cpu().numpy())
    np.testing.assert_array_equal(c.ob64[0].cpu().numpy(), ob.cpu().numpy())                 # carried over as the next segment's first row
    with pytest.raises(ValueError):
        SegmentCollector(pi, env, T, fused=True)
    with pytest.raises(ValueError):
        SegmentCollector(MlpPolicy(device=DEV, seed=1), env, T, fused=True)                  # a 56-wide native policy does not make it fusable
    with pytest.raises(ValueError):
        RolloutBlock(2, n, device=DEV).append(ob, ac64[0], rew, done)
    from deepmimic_mujoco_amd.rollout import DoubleBufferedGather
    with pytest.raises(ValueError):
        DoubleBufferedGather(2, n, device=DEV, ob_width=env.observation_space.shape[0])
    assert DoubleBufferedGather(2, n, device=DEV).blocks[0].shape == (2, n, 87)
    env.close(); twin.close()


# ---- training end to end at width 171 -------------------------------------------------------------------------------------------------------
def run_tool(args, timeout=900):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def all_finite(hist):
    vals = [x for h in hist for x in h.values() if isinstance(x, (int, float))]
    return len(vals) > 0 and bool(np.isfinite(np.asarray(vals, dtype=np.float64)).all())


def test_trpo_and_ppo_train_through_the_tools(tmp_path):
    common = ["--envs", "256", "--horizon", "32", "--reward", "imitation", "--autoreset", "rsi", "--obs-mode", "deepmimic"]
    out, ckpt = str(tmp_path / "trpo.json"), str(tmp_path / "trpo.npz")
    run_tool([os.path.join(ROOT, "tools", "train_trpo.py"), "--iters", "2", "--out", out, "--save", ckpt] + common)
    hist = json.load(open(out))["history"]
    assert len(hist) == 2 and all_finite(hist), hist
    pi = MlpPolicy.from_npz(ckpt, device=DEV)
    assert pi.ob_dim == 171 and tuple(pi.ob_rms.shape) == (171,)
    txt = run_tool([os.path.join(ROOT, "tools", "train_trpo.py"), "--task", "evaluate", "--load-model-path", ckpt, "--number-trajs", "4", "--reward", "imitation",
                    "--obs-mode", "deepmimic"])
    assert "Average length" in txt
    out, ckpt = str(tmp_path / "ppo.json"), str(tmp_path / "ppo")
    run_tool([os.path.join(ROOT, "tools", "train_ppo.py"), "--iters", "1", "--optim-epochs", "1", "--out", out, "--save", ckpt] + common)
    hist = json.load(open(out))["history"]
    assert len(hist) == 1 and all_finite(hist), hist
    assert MlpPolicy.from_tf_checkpoint(ckpt, device=DEV).ob_dim == 171


def test_gail_trains_through_the_tool(tmp_path):
    """expert samples at width 171 from a freshly initialised policy, then one GAIL iteration on the torch paths"""
    ckpt, sample, out = str(tmp_path / "pi.npz"), str(tmp_path / "expert.npz"), str(tmp_path / "gail.json")
    MlpPolicy(ob_dim=171, device=DEV, seed=3).save_npz(ckpt)
    run_tool([os.path.join(ROOT, "tools", "train_trpo.py"), "--task", "evaluate", "--load-model-path", ckpt, "--number-trajs", "8", "--obs-mode", "deepmimic",
              "--save-sample", sample])
    run_tool([os.path.join(ROOT, "tools", "train_gail.py"), "--expert-path", sample, "--envs", "256", "--horizon", "16", "--iters", "1", "--obs-mode", "deepmimic",
              "--out", out, "--save", str(tmp_path / "gail.npz")])
    hist = json.load(open(out))["history"]
    assert len(hist) == 1 and all_finite(hist), hist
    assert MlpPolicy.from_npz(str(tmp_path / "gail.npz"), device=DEV).ob_dim == 171
