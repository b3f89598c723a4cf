"""The truncation log and the value bootstrap at a time-limit end, on the GPU: k_terminate's records against twin batches that
never met a limit, what gets no record, overflow / clear / resizing, the log off against on in every launch form, k_gae_boot against the float64
restatement (tests/gae_numpy.py), the segment collector's "vboot", and a short training call of each learner.

Bars.  A record is a copy of the state the step left: bit for bit the twin's.  GAE: the tolerances tests/test_learner_reference.py uses (rtol 2e-5,
atol 2e-4: float32 recursions against float64).  A bootstrap value is the float32 value net evaluated in another batch shape than the check evaluates
it in: 256 accumulations of float32 products per row, |v| of order 1 — rtol 1e-4, atol 1e-5.

The inputs of the record tests: exact `walk` frames, actions 0.1 N(0, 1) from RandomState(11).  The CPU oracle steps all 66 of these environments
through 6 steps without the step's own done, so every environment reaches the limit at its 3rd step; the test asserts at least three quarters."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
from deepmimic_mujoco_amd import termination as TM
from deepmimic_mujoco_amd.rollout import SegmentCollector, add_vtarg_and_adv, pipelined_segment_generator
from deepmimic_mujoco_amd.state_features import phase_of
from tests import floor_numpy as FN
from tests import helpers as H
from tests.gae_numpy import gae_boot, random_segment
from tests.gpu_batch import DEV, put_state, start, state_of, step_numpy, truncation_log

pytestmark = pytest.mark.gpu
SEED = 5
M = 3
STEPS = 7
RTOL, ATOL = 2e-5, 2e-4

FORMS = {
    "one-env-6": dict(n=6),
    "one-env-6-pipe2": dict(n=6, pipeline=2),
    "packed-66": dict(n=66, packed=True),                      # 17 waves, the last one partial
    "packed-66-pipe2": dict(n=66, packed=True, pipeline=2),
}


def make(n, limit=0, log=0, fall=None, autoreset=None, dtype=64, packed=False, pipeline=1, reward="alive"):
    env = DPVecEnv(n, motion="walk", reward=reward, autoreset=autoreset, seed=SEED, dtype=dtype, packed=packed, fall_contact_bodies=fall,
                   max_episode_steps=limit, truncation_log=log)
    if pipeline > 1:
        env.batch.set_option(A.OPT_PIPELINE, pipeline)
    assert env.packed or not packed
    return env


def frames_start(n):
    mc = H.mocap("walk")
    idx = (np.arange(n) * 5 % mc.data_config.shape[0]).astype(np.int32)
    return idx, mc.data_config[idx].copy(), mc.data_vel[idx].copy()


# ---- records against a twin; the log off against on --------------------------------------------------------------------------------------------
CASES = [(f, ar, host, 64) for f in sorted(FORMS) for ar in (None, "rsi", "init") for host in (False, True)] + [(f, "rsi", False, 32) for f in sorted(FORMS)]


@pytest.mark.parametrize("form,autoreset,host,dtype", CASES)
def test_records_against_a_twin_and_off_is_off(form, autoreset, host, dtype):
    cfg = dict(FORMS[form]); n = cfg.pop("n")
    idx, q, v = frames_start(n)
    acts = np.random.RandomState(11).randn(STEPS, n, 28) * 0.1
    on = make(n, limit=M, log=3 * n, autoreset=autoreset, dtype=dtype, **cfg)          # at most 3 truncations per env in 7 steps
    off = make(n, limit=M, autoreset=autoreset, dtype=dtype, **cfg)                    # the same run, the log off
    twin = make(n, dtype=dtype, **cfg)                                                 # no limit, no auto-reset: the states a limit would cut off
    for e in (on, off, twin):
        start(e.batch, idx, q, v)
    expect = []                        # (tick, env, qpos, qvel, frame_idx, frame_init) from the twin
    compared = [0, 0]
    own_done = np.zeros(n, dtype=bool)
    for t in range(STEPS):
        o1, r1, d1 = step_numpy(on.batch, acts[t], host=host)
        o0, r0, d0 = step_numpy(off.batch, acts[t], host=host)
        for x, y in ((o1, o0), (r1, r0), (d1, d0)):
            np.testing.assert_array_equal(x, y)                                        # off is off: the log changes nothing a caller sees ...
        reason = on.batch.get(A.F_DONE_REASON)
        np.testing.assert_array_equal(reason, off.batch.get(A.F_DONE_REASON))
        np.testing.assert_array_equal(on.batch.get(A.F_EPISODE_STEPS), off.batch.get(A.F_EPISODE_STEPS))
        if t < 6:
            _o, _r, dt = step_numpy(twin.batch, acts[t], host=host)
            own_done |= dt != 0
        if t in (2, 5):
            # every env whose own done stayed 0 since the (re)start is truncated here, and its record is the twin's state
            ok = ~own_done
            assert ok.sum() * 4 >= 3 * n if t == 2 else ok.sum() * 2 >= n, (t, int(ok.sum()))
            np.testing.assert_array_equal(reason[ok], np.full(int(ok.sum()), TM.DONE_TIME_LIMIT))
            st = state_of(twin.batch)
            for e in np.nonzero(ok)[0]:
                expect.append((t, int(e), st[A.F_QPOS][e].copy(), st[A.F_QVEL][e].copy(), int(st[A.F_FRAME_IDX][e]), int(st[A.F_FRAME_INIT][e])))
            compared[0 if t == 2 else 1] = int(ok.sum())
            # the twin goes on from the batch's own state after the step (with auto-reset: the fresh episodes)
            put_state(twin.batch, state_of(on.batch), np.zeros(n, dtype=np.int32))
            own_done = on.batch.get(A.F_EPISODE_STEPS) != 0                            # (an env whose counter is not at 0 now reaches the limit on another row)
    s1, s0 = state_of(on.batch), state_of(off.batch)
    for f in s1:
        np.testing.assert_array_equal(s1[f], s0[f])                                    # ... and nothing in the batch's state
    count, ridx, rq, rv = truncation_log(on.batch, host=host, device=not host)
    assert count == len(ridx) <= 3 * n
    got = {(int(r[1]), int(r[0])): k for k, r in enumerate(ridx)}
    assert len(got) == count                                                            # (tick, env) is a key
    for t, e, eq, ev, fi, fin in expect:
        k = got[(t, e)]
        np.testing.assert_array_equal(rq[k], eq); np.testing.assert_array_equal(rv[k], ev)
        assert (int(ridx[k, 2]), int(ridx[k, 3])) == (fi, fin)
    assert set(t for t, _e in got) <= {2, 3, 4, 5, 6} and len(expect) >= n                # (an env whose own done restarted its counter is truncated later)
    print("%s / %s / %s / float%d: %d records, %d + %d compared with the twin" % (form, autoreset, "host" if host else "device", dtype, count, compared[0], compared[1]))
    with pytest.raises(A.DmenvError):
        off.batch.truncations()                                                         # the log is off there: DM_EINVAL
    assert off.batch._L.dm_batch_truncations(off.batch._h, A.C.c_void_p(np.zeros(1, dtype=np.int32).ctypes.data), None, None, None, 0, 0, A.PTR_HOST) == -1
    for e in (on, off, twin):
        e.close()


# ---- what gets no record -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_no_record_for_a_step_done_or_a_fall_at_the_limit_step(packed):
    """Every env is on its limit step (the counter planted at M - 1).  Of the varied states some are ended by the step itself and some have a fall body in
    the floor once the step is over (every other exact frame is sunk 0.10 m, as tests/test_gpu_termination.py plants them): neither kind gets a record."""
    n = 66 if packed else 48
    cm = H.compiled_model()
    idx, q, v, _ws, _c = H.varied_states(n, seed=7)
    q[0::8, 2] -= 0.10
    a = np.random.RandomState(1).randn(n, 28) * 0.9
    plain = make(n, packed=packed)
    on = make(n, limit=M, log=n, fall="deepmimic", autoreset="rsi", packed=packed)
    start(plain.batch, idx, q, v); start(on.batch, idx, q, v, steps0=np.full(n, M - 1, dtype=np.int32))
    _o, _r, d0 = step_numpy(plain.batch, a)
    step_numpy(on.batch, a)
    left = state_of(plain.batch)
    stepdone = d0 != 0
    gm = TM.geoms_of_bodies(TM.fall_body_mask("deepmimic"), cm.geom_bodyid)
    fall = ((FN.floor_masks(cm, left[A.F_QPOS]) & gm) != 0) & ~stepdone
    trunc = ~stepdone & ~fall
    assert stepdone.any() and fall.sum() >= max(1, n // 16) and trunc.sum() >= n // 8
    np.testing.assert_array_equal(on.batch.get(A.F_DONE_REASON),
                                  np.where(stepdone, TM.DONE_STEP, np.where(fall, TM.DONE_FALL | TM.DONE_TIME_LIMIT, TM.DONE_TIME_LIMIT)))
    count, ridx, rq, rv = truncation_log(on.batch, host=True)
    np.testing.assert_array_equal(ridx[:, 0], np.nonzero(trunc)[0])                     # exactly the envs the limit alone ended
    assert count == trunc.sum() and not ridx[:, 1].any()
    np.testing.assert_array_equal(rq, left[A.F_QPOS][trunc]); np.testing.assert_array_equal(rv, left[A.F_QVEL][trunc])
    np.testing.assert_array_equal(ridx[:, 2], left[A.F_FRAME_IDX][trunc]); np.testing.assert_array_equal(ridx[:, 3], left[A.F_FRAME_INIT][trunc])
    plain.close(); on.close()


def test_no_record_without_a_time_limit():
    """the option has an effect only while DM_OPT_MAX_EPISODE_STEPS > 0: falls alone leave the log empty"""
    n = 48
    idx, q, v, _ws, _c = H.varied_states(n, seed=7)
    q[0::8, 2] -= 0.10
    env = make(n, log=n, fall="deepmimic", autoreset="rsi")
    start(env.batch, idx, q, v)
    step_numpy(env.batch, np.random.RandomState(1).randn(n, 28) * 0.9)
    assert (env.batch.get(A.F_DONE_REASON) == TM.DONE_FALL).any()
    assert truncation_log(env.batch, host=True)[0] == 0
    env.close()


# ---- overflow, clear, resizing -------------------------------------------------------------------------------------------------------------------
def test_overflow_clear_and_resizing():
    n = 6
    env = make(n, limit=1, log=4, autoreset="init")
    b = env.batch
    b.reset(mode=2, hard=1)
    a = np.zeros((n, 28))
    _o, _r, d = step_numpy(b, a)
    assert (d != 0).all() and (b.get(A.F_DONE_REASON) == TM.DONE_TIME_LIMIT).all()
    guard = -7
    out = (np.full(1, guard, dtype=np.int32), np.full((6, 4), guard, dtype=np.int32), np.full((6, 35), float(guard)), np.full((6, 34), float(guard)))
    cnt, idx, qp, qv = b.truncations(clear=False, out=out)
    assert int(cnt[0]) == 6                                                             # the counter keeps counting: the overflow is visible
    assert (idx[4:] == guard).all() and (qp[4:] == guard).all() and (qv[4:] == guard).all()    # nothing beyond the log's four rows is written
    assert len(set(idx[:4, 0])) == 4 and set(idx[:4, 0]) <= set(range(n)) and not idx[:4, 1].any()
    assert np.isfinite(qp[:4]).all() and (qp[:4, 2] > 0.5).all()                           # standing states, not the guard
    small = (np.zeros(1, dtype=np.int32), np.full((2, 4), guard, dtype=np.int32), None, None)
    cnt2, idx2, _q, _v = b.truncations(clear=False, out=small)                          # a smaller cap, two of the arrays left out
    assert int(cnt2[0]) == 6
    np.testing.assert_array_equal(idx2, idx[:2])
    # without a clear the tick goes on; with one, count and tick start again
    step_numpy(b, a)
    cnt, idx, _q, _v = b.truncations(clear=True, device=False)
    assert int(cnt[0]) == 12 and not idx[:4, 1].any()                                   # (the four stored records are still the first four)
    cnt, _i, _q, _v = b.truncations(clear=False, device=False)
    assert int(cnt[0]) == 0
    step_numpy(b, a)
    count, ridx, _q, _v = truncation_log(b, host=True)
    assert count == 6 and len(ridx) == 4 and not ridx[:, 1].any()                       # tick 0 again
    # device pointers: the same numbers, nothing waits
    step_numpy(b, a)
    count, ridx, _q, _v = truncation_log(b, device=True)
    assert count == 12 and len(ridx) == 4
    # resizing clears
    b.set_option(A.OPT_TRUNCATION_LOG, 8)
    assert truncation_log(b, host=True)[0] == 0
    step_numpy(b, a)
    count, ridx, rq, _v = truncation_log(b, host=True)
    assert count == 6 and sorted(ridx[:, 0]) == list(range(n)) and not ridx[:, 1].any()
    with pytest.raises(A.DmenvError):
        b.set_option(A.OPT_TRUNCATION_LOG, -1)
    L = b._L
    p = lambda x: A.C.c_void_p(x.ctypes.data)
    c1 = np.zeros(1, dtype=np.int32)
    assert L.dm_batch_truncations(b._h, None, None, None, None, 0, 0, A.PTR_HOST) == -1            # no count
    assert L.dm_batch_truncations(b._h, p(c1), None, None, None, -1, 0, A.PTR_HOST) == -1          # cap < 0
    assert L.dm_batch_truncations(b._h, p(c1), None, None, None, 0, 0, 7) == -1                    # bad ptr_kind
    assert L.dm_batch_truncations(b._h, p(c1), None, None, None, 0, 0, A.PTR_HOST) == 0 and int(c1[0]) == 6
    b.set_option(A.OPT_TRUNCATION_LOG, 0)
    with pytest.raises(A.DmenvError):
        b.truncations()
    env.close()


# ---- dm_gae_boot -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_gae_boot_kernel(T, n):
    gamma, lam = 0.99, 0.95
    seg = random_segment(T, n, seed=1000 * T + n)
    dev = {k: torch.as_tensor(x, device=DEV) for k, x in seg.items()}
    want_adv, want_ret = gae_boot(seg["rew"], seg["vpred"], seg["new"], seg["nextvpred"], seg["vboot"], gamma, lam)
    got = add_vtarg_and_adv(dict(dev), gamma, lam)
    assert got["adv"].is_cuda and got["adv"].dtype == torch.float32
    assert np.allclose(got["adv"].cpu().numpy(), want_adv, rtol=RTOL, atol=ATOL) and np.allclose(got["tdlamret"].cpu().numpy(), want_ret, rtol=RTOL, atol=ATOL)
    plain_adv, _ = gae_boot(seg["rew"], seg["vpred"], seg["new"], seg["nextvpred"], None, gamma, lam)
    assert np.abs(want_adv - plain_adv).max() > 0.5                                     # (the bootstrap is in the numbers)
    # vboot = 0: dm_gae's outputs bit for bit
    no_key = {k: x for k, x in dev.items() if k != "vboot"}
    plain = add_vtarg_and_adv(dict(no_key), gamma, lam)
    zero = add_vtarg_and_adv(dict(no_key, vboot=torch.zeros((T, n), dtype=torch.float32, device=DEV)), gamma, lam)
    assert torch.equal(zero["adv"], plain["adv"]) and torch.equal(zero["tdlamret"], plain["tdlamret"])
    assert np.allclose(plain["adv"].cpu().numpy(), plain_adv, rtol=RTOL, atol=ATOL)


def test_gae_boot_is_dm_gae_on_the_reference_fixture_with_zero_vboot():
    import os
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "learner_ref_golden.npz"))
    seg = {k: torch.as_tensor(G["gae_" + k], device=DEV) for k in ("rew", "vpred", "new", "nextvpred")}
    gamma, lam = (float(x) for x in G["gae_gamma_lam"])
    plain = add_vtarg_and_adv(dict(seg), gamma, lam)
    zero = add_vtarg_and_adv(dict(seg, vboot=torch.zeros_like(seg["rew"])), gamma, lam)
    assert torch.equal(zero["adv"], plain["adv"]) and torch.equal(zero["tdlamret"], plain["tdlamret"])
    assert np.allclose(zero["adv"].cpu().numpy(), G["gae_adv"], rtol=RTOL, atol=ATOL)


# ---- the collector -----------------------------------------------------------------------------------------------------------------------------------
def collector(obs_mode, fused, flag, n=66, T=7, limit=M):
    env = DPVecEnv(n, motion="walk", autoreset="init", seed=SEED, obs_mode=obs_mode, max_episode_steps=limit)
    pi = MlpPolicy(ob_dim=env.observation_space.shape[0], device=DEV, seed=3); pi.seed(4)
    return env, pi, SegmentCollector(pi, env, T, fused=fused, bootstrap_time_limit=flag)


@pytest.mark.parametrize("obs_mode,fused", [("dp_env_v3", True), ("dp_env_v3", False), ("deepmimic", False)])
def test_collector_bootstrap_values(obs_mode, fused):
    n, T = 66, 7
    gamma, lam = 0.99, 0.95
    env, pi, c = collector(obs_mode, fused, True)
    b = env.batch
    assert b.options[A.OPT_TRUNCATION_LOG] == n * (T // M + 1)
    c.launch()
    seg = c.collect()
    vboot = seg["vboot"]
    assert vboot.is_cuda and vboot.dtype == torch.float32 and tuple(vboot.shape) == (T, n)
    count, ridx, rq, rv = truncation_log(b, device=True)
    assert seg.trunc_count() == count == len(ridx) and n <= count <= 2 * n               # most envs are truncated at rows 2 and 5
    # the record's observation, and the critic's value of it
    if obs_mode == "dp_env_v3":
        ob = np.concatenate([rq[:, 7:], rv[:, 6:]], 1)
    else:
        ob = b.state_features(qpos=rq, qvel=rv, phase=phase_of(0, ridx[:, 2], ridx[:, 3], b.n_frames))
    with torch.no_grad():
        want = pi.forward_value(torch.as_tensor(ob, device=DEV)).cpu().numpy()
    got = vboot.cpu().numpy()
    where = np.zeros((T, n), dtype=bool)
    where[ridx[:, 1], ridx[:, 0]] = True
    np.testing.assert_array_equal(got != 0, where)                                      # non-zero exactly at the records' (tick, env)
    assert np.allclose(got[ridx[:, 1], ridx[:, 0]], want, rtol=1e-4, atol=1e-5)
    new = seg["new"].cpu().numpy()
    assert (new[1:][where[:-1]] != 0).all() and (c.first.cpu().numpy()[where[-1]] != 0).all()      # a truncation ends its episode
    assert where[2].sum() * 4 >= 3 * n                                                  # (row 2: the limit's first turn)
    host = {k: seg[k].cpu().numpy() for k in ("rew", "vpred", "new", "nextvpred", "vboot")}
    add_vtarg_and_adv(seg, gamma, lam)
    want_adv, want_ret = gae_boot(host["rew"], host["vpred"], host["new"], host["nextvpred"], host["vboot"], gamma, lam)
    assert np.allclose(seg["adv"].cpu().numpy(), want_adv, rtol=RTOL, atol=ATOL) and np.allclose(seg["tdlamret"].cpu().numpy(), want_ret, rtol=RTOL, atol=ATOL)
    # the flag off: no "vboot", and every other entry is what the flagged collector produced
    env0, pi0, c0 = collector(obs_mode, fused, False)
    c0.launch()
    seg0 = c0.collect()
    assert "vboot" not in seg0 and seg0.trunc_count() is None
    for k in ("ob", "rew", "vpred", "new", "ac", "prevac", "nextvpred"):
        assert torch.equal(seg0[k], seg[k]), k
    assert seg0["ep_lens"] == seg["ep_lens"]
    add_vtarg_and_adv(seg0, gamma, lam)
    plain_adv, _ = gae_boot(host["rew"], host["vpred"], host["new"], host["nextvpred"], None, gamma, lam)
    assert np.allclose(seg0["adv"].cpu().numpy(), plain_adv, rtol=RTOL, atol=ATOL)
    # a second segment: the log was cleared at its launch, ticks count from its first step
    c.launch()
    seg2 = c.collect()
    count2, ridx2, _q, _v = truncation_log(b, device=True)
    assert seg2.trunc_count() == count2 and ridx2[:, 1].max() < T and (seg2["vboot"] != 0).sum().item() == count2
    env.close(); env0.close()


def test_collector_flag_needs_a_time_limit():
    env = DPVecEnv(6, motion="walk", autoreset="init", seed=SEED)
    pi = MlpPolicy(device=DEV, seed=3)
    with pytest.raises(ValueError):
        SegmentCollector(pi, env, 7, bootstrap_time_limit=True)
    env.close()


def test_pipelined_generator_joins_vboot_along_the_env_axis():
    T, gamma, lam = 7, 0.99, 0.95
    envs = [DPVecEnv(n, motion="walk", autoreset="init", seed=SEED + k, max_episode_steps=M) for k, n in enumerate((6, 10))]
    pi = MlpPolicy(device=DEV, seed=3); pi.seed(4)
    seg = next(pipelined_segment_generator(pi, envs, T, bootstrap_time_limit=True))
    assert tuple(seg["vboot"].shape) == (T, 16) == tuple(seg["rew"].shape)
    nz = (seg["vboot"] != 0).cpu().numpy()
    assert seg.trunc_count() == nz.sum() >= 16 and nz[:, :6].any() and nz[:, 6:].any()
    host = {k: seg[k].cpu().numpy() for k in ("rew", "vpred", "new", "nextvpred", "vboot")}
    add_vtarg_and_adv(seg, gamma, lam)
    want_adv, _ = gae_boot(host["rew"], host["vpred"], host["new"], host["nextvpred"], host["vboot"], gamma, lam)
    assert np.allclose(seg["adv"].cpu().numpy(), want_adv, rtol=RTOL, atol=ATOL)
    for e in envs:
        e.close()


# ---- a short training call ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["trpo", "ppo", "gail"])
def test_learners_run_with_the_flag(algo):
    n, T = 66, 8
    env = DPVecEnv(n, motion="walk", autoreset="init", seed=SEED, max_episode_steps=M)
    pi = MlpPolicy(device=DEV, seed=1); pi.seed(1)
    if algo == "trpo":
        from deepmimic_mujoco_amd.trpo import learn
        hist = learn(env, pi, timesteps_per_batch=T, max_iters=2, log=None, seed=1, bootstrap_time_limit=True)
    elif algo == "ppo":
        from deepmimic_mujoco_amd.ppo import learn
        hist = learn(env, pi, timesteps_per_batch=T, max_iters=2, log=None, seed=1, schedule="constant", optim_epochs=2, optim_batchsize=64,
                     bootstrap_time_limit=True)
    else:
        from deepmimic_mujoco_amd.gail import ExpertDataset, TransitionClassifier, learn
        rng = np.random.RandomState(0)
        expert = ExpertDataset(dict(obs=rng.randn(4, 40, 56).astype(np.float32), acs=rng.randn(4, 40, 28).astype(np.float32), ep_rets=np.ones(4), lens=np.full(4, 40)),
                               seed=0, device=DEV)
        rg = TransitionClassifier(device=DEV, seed=1)
        hist = learn(env, pi, rg, expert, g_step=1, d_step=1, timesteps_per_batch=T, max_iters=2, log=None, seed=1, bootstrap_time_limit=True)
    assert len(hist) == 2
    for h in hist:
        assert n <= h["TruncThisIter"] <= n * (T // M + 1)
        keys = {"trpo": ("meankl", "surrgain", "entropy"), "ppo": ("loss_pol_surr", "loss_vf_loss", "loss_kl"), "gail": ("meankl", "generator_loss", "expert_loss")}[algo]
        assert all(np.isfinite(h[k]) for k in keys + ("ev_tdlam_before", "EpLenMean", "EpRewMean")), h
        assert h["EpThisIter"] >= n and h["EpLenMean"] <= M
    env.close()
