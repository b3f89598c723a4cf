"""Early termination on the GPU (csrc/term_kernel.h): dm_batch_floor_contacts against the float64 restatement (tests/floor_numpy.py) and
against the step's own contact list, and k_terminate behind every per-step launch form — twin batches with the options off and on.

Bars.  The query's answer is a set of bits: the float64 library must give the restatement's exactly; the float32 library may differ on
(state, geom) pairs within 1e-4 m of the decision boundary, of which there may be at most 0.5 % (tests/test_termination.py has the
count for the inputs: 0.09 %).  Everything k_terminate leaves alone is compared bit for bit with the twin that never ran it; what it
writes (done, reason, counter, the fresh episode's state and observation row) is predicted on the host."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch, DPEnv, DPVecEnv
from deepmimic_mujoco_amd import termination as T
from tests import floor_numpy as FN
from tests import helpers as H
from tests import state_numpy as SN
from tests.gpu_batch import DEV, fused_policy, horizon_rows, put_state, start, state_of, step_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEAR_CAP = 0.005
SEED = 5
DEEPMIMIC = T.fall_body_mask("deepmimic")


def geom_mask(bodies=DEEPMIMIC):
    return T.geoms_of_bodies(bodies, H.compiled_model().geom_bodyid)


def make(n, fall=0, limit=0, dtype=64, clip="walk", reward="alive", autoreset=None, packed=False, pipeline=1, action_mode="raw", step_queue=0, diagnostics=False):
    env = DPVecEnv(n, motion=clip, reward=reward, autoreset=autoreset, seed=SEED, dtype=dtype, packed=packed, action_mode=action_mode,
                   step_queue=step_queue, diagnostics=diagnostics, fall_contact_bodies=fall or None, max_episode_steps=limit)
    if pipeline > 1:
        env.batch.set_option(A.OPT_PIPELINE, pipeline)
    assert env.packed or not packed
    return env


def states(n, seed):
    """helpers.varied_states, with every other exact mocap frame among them (env 0, 8, 16, ...) sunk 0.10 m into the floor: the lower ends of the shin
    capsules then touch it while the centre of mass stays inside the step's own band — without them no state here falls that the step does not end itself"""
    idx, q, v, _ws, _c = H.varied_states(n, seed=seed)
    q[0::8, 2] -= 0.10
    return idx, q, v


# ---- the query --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_query_on_explicit_states(dtype):
    cm = H.compiled_model()
    q, _v = FN.query_states()
    gap = FN.query_gaps(cm)
    env = make(4, dtype=dtype)
    b = env.batch
    got = b.floor_contacts(qpos=q)
    assert got.dtype == np.int32 and got.shape == (len(q),)
    wrong, near = FN.compare(got, gap)
    differ = int((got != FN.masks_of(gap)).sum())
    print("float%d query: %d of %d pairs within %.0e m of the boundary, %d states answered differently" % (dtype, near, gap[:, 1:].size, FN.BAND, differ))
    if dtype == 64:
        np.testing.assert_array_equal(got, FN.masks_of(gap))
    assert near <= NEAR_CAP * gap[:, 1:].size
    assert not wrong, wrong[:10]
    out = torch.zeros(len(q), dtype=torch.int32, device=DEV)
    assert b.floor_contacts(qpos=torch.as_tensor(q, device=DEV), out=out) is out
    np.testing.assert_array_equal(out.cpu().numpy(), got)                          # host and device pointers: the same launch
    env.close()


def test_query_on_the_batch_state_is_the_steps_floor_contact_list():
    n = 48
    env = make(n, diagnostics=True)
    b = env.batch
    idx, q, v, _ws, _c = H.varied_states(n, seed=3)
    before = state_of(b)
    b.set_state(q, v, frame_idx=idx)
    cg = b.get(A.F_CONTACT_GEOMS)
    ncon = b.get(A.F_NCON)
    assert ncon.max() <= A.MAXEFC
    want = np.zeros(n, dtype=np.int32)
    for e in range(n):
        for g1, g2 in cg[e]:
            if g1 == 0:
                want[e] |= 1 << int(g2)
    before = state_of(b)
    got = b.floor_contacts()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, FN.floor_masks(H.compiled_model(), q))
    assert np.count_nonzero(got) > n // 4
    ids = np.array([5, 0, 47, 5, 13], dtype=np.int32)
    np.testing.assert_array_equal(b.floor_contacts(env_ids=ids), want[ids])
    np.testing.assert_array_equal(b.floor_contacts(env_ids=torch.as_tensor(ids, device=DEV)).cpu().numpy(), want[ids])
    after = state_of(b)
    for f in before:
        np.testing.assert_array_equal(before[f], after[f])                          # read-only
    env.close()


def test_query_argument_errors():
    env = make(4)
    b, L = env.batch, env.batch._L
    q = np.zeros((2, 35)); out = np.zeros(8, dtype=np.int32); ids = np.zeros(2, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(A.C.c_void_p)
    assert L.dm_batch_floor_contacts(b._h, None, None, 2, None, A.PTR_HOST) == -1                 # no output
    assert L.dm_batch_floor_contacts(b._h, None, None, 0, p(out), A.PTR_HOST) == -1               # n <= 0
    assert L.dm_batch_floor_contacts(b._h, None, None, 5, p(out), A.PTR_HOST) == -1               # n beyond the batch
    assert L.dm_batch_floor_contacts(b._h, p(q), p(ids), 2, p(out), A.PTR_HOST) == -1             # env_ids with explicit states
    assert L.dm_batch_floor_contacts(b._h, None, None, 2, p(out), 7) == -1                        # bad ptr_kind
    for bad in ([0, 4], [-1, 0]):
        assert L.dm_batch_floor_contacts(b._h, None, p(np.array(bad, dtype=np.int32)), 2, p(out), A.PTR_HOST) == -1 and b"out of range" in L.dm_last_error()
    with pytest.raises(ValueError):
        b.floor_contacts(qpos=q, env_ids=ids)
    for opt, bad in ((A.OPT_FALL_BODIES, 1), (A.OPT_FALL_BODIES, 1 << 14), (A.OPT_FALL_BODIES, -2), (A.OPT_MAX_EPISODE_STEPS, -1)):
        with pytest.raises(A.DmenvError):
            b.set_option(opt, bad)
    with pytest.raises(ValueError):
        DPVecEnv(4, fall_contact_bodies=["pelvis"])
    env.close()


# ---- one step from varied states: twins with the options off and on -------------------------------------------------------------------------
FORMS = {
    "one-env": dict(n=48),
    "packed-66": dict(n=66, packed=True),
    "packed-pipe2-6": dict(n=6, packed=True, pipeline=2),
    "packed-pipe2-66": dict(n=66, packed=True, pipeline=2),
    "one-env-pipe2": dict(n=48, pipeline=2),
    "host-pointers": dict(n=48, host=True),
    "imitation": dict(n=48, reward="imitation"),
    "imitation-packed": dict(n=66, reward="imitation", packed=True),
    "spd-target": dict(n=48, action_mode="spd-target"),
    "float32": dict(n=48, dtype=32),
}
LIMIT = 3


def fresh_state(b, mode, env, episode, dtype):
    """what reset_env leaves for (seed, env, episode): (frame, qpos, qvel)"""
    mc = H.mocap("walk")
    F = mc.data_config.shape[0]
    k = H.device_rsi_frame(SEED, env, episode, F)
    R = np.float64 if dtype == 64 else np.float32
    if mode == "rsi":
        return k, mc.data_config[k].astype(R).astype(np.float64), mc.data_vel[k].astype(R).astype(np.float64)
    q0 = H.compiled_model().qpos0.astype(R)
    dq = np.array([(H.device_rng_uniform(SEED, env, episode, 1 + l) * 2.0 - 1.0) * 0.01 for l in range(35)]).astype(R)
    dv = np.array([(H.device_rng_uniform(SEED, env, episode, 64 + l) * 2.0 - 1.0) * 0.01 for l in range(34)]).astype(R)
    return k, (q0 + dq).astype(np.float64), dv.astype(np.float64)


@pytest.mark.parametrize("autoreset", [None, "rsi", "init"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_one_step_against_the_twin_without_termination(form, autoreset):
    cfg = dict(FORMS[form])
    n, host = cfg.pop("n"), cfg.pop("host", False)
    dtype = cfg.get("dtype", 64)
    cm = H.compiled_model()
    idx, q, v = states(n, seed=7)
    rng = np.random.RandomState(1)
    a = rng.randn(n, 28) * 0.9
    if cfg.get("action_mode") == "spd-target":
        a = q[:, 7:] + 0.1 * rng.randn(n, 28)
    steps0 = (np.arange(n) % LIMIT).astype(np.int32)                 # a third of the envs reach the limit on this step
    off = make(n, autoreset=autoreset, **cfg)
    on = make(n, fall="deepmimic", limit=LIMIT, autoreset=autoreset, **cfg)
    start(off.batch, idx, q, v); start(on.batch, idx, q, v, steps0=steps0)
    ep0 = on.batch.get(A.F_EPISODE)
    o0, r0, d0 = step_numpy(off.batch, a, host=host)
    o1, r1, d1 = step_numpy(on.batch, a, host=host)
    s0, s1 = state_of(off.batch), state_of(on.batch)
    # the fall test on the state the step left (the off twin's, where the step did not end the episode itself)
    touch = FN.floor_masks(cm, s0[A.F_QPOS]) if dtype == 64 else off.batch.floor_contacts()
    if dtype == 64:
        np.testing.assert_array_equal(off.batch.floor_contacts(), touch)
    stepdone = d0 != 0
    fall = ((touch & geom_mask()) != 0) & ~stepdone
    limit = (steps0 + 1 >= LIMIT) & ~stepdone
    term = fall | limit
    print("%s / %s: %d envs, %d ended by the step, %d fell, %d at the limit" % (form, autoreset, n, stepdone.sum(), fall.sum(), limit.sum()))
    assert fall.sum() >= max(1, n // 16) and limit.sum() >= max(1, n // 8) and (~term & ~stepdone).sum() >= max(1, n // 8) and stepdone.any()
    np.testing.assert_array_equal(d1 != 0, stepdone | term)
    np.testing.assert_array_equal(on.batch.get(A.F_DONE_REASON), np.where(stepdone, T.DONE_STEP, fall * T.DONE_FALL + limit * T.DONE_TIME_LIMIT))
    np.testing.assert_array_equal(on.batch.get(A.F_EPISODE_STEPS), np.where(stepdone | term, 0, steps0 + 1))
    np.testing.assert_array_equal(r1, r0)                            # the reward is left as the step wrote it
    keep = ~term if autoreset else np.ones(n, dtype=bool)            # without auto-reset nothing but done / reason / counter moves
    np.testing.assert_array_equal(o1[keep], o0[keep])
    for f in s0:
        np.testing.assert_array_equal(s1[f][keep], s0[f][keep])
    if autoreset:
        cyc_mode = cfg.get("reward", "alive")
        for e in np.nonzero(term)[0]:
            k, fq, fv = fresh_state(on.batch, autoreset, int(e), int(ep0[e]), dtype)
            np.testing.assert_array_equal(s1[A.F_QPOS][e], fq); np.testing.assert_array_equal(s1[A.F_QVEL][e], fv)
            np.testing.assert_array_equal(o1[e], np.concatenate([fq[7:], fv[6:]]))
            assert s1[A.F_EPISODE][e] == ep0[e] + 1 and s1[A.F_FRAME_IDX][e] == k and s1[A.F_FRAME_INIT][e] == k and s1[A.F_CYCLE][e] == 0, (e, cyc_mode)
            assert s1[A.F_TIME][e] == 0 and not s1[A.F_QACC_WARMSTART][e].any()
        # parked kinematics of the old state are not used: one more step agrees with a twin that was SET to the state the batch is in
        twin = make(n, fall="deepmimic", limit=LIMIT, autoreset=autoreset, **cfg)
        tb = twin.batch
        put_state(tb, s1, on.batch.get(A.F_EPISODE_STEPS))
        a2 = rng.randn(n, 28) * 0.9 if cfg.get("action_mode") != "spd-target" else s1[A.F_QPOS][:, 7:] + 0.1 * rng.randn(n, 28)
        o2, r2, d2 = step_numpy(on.batch, a2, host=host)
        o3, r3, d3 = step_numpy(tb, a2, host=host)
        np.testing.assert_array_equal(o2, o3); np.testing.assert_array_equal(r2, r3); np.testing.assert_array_equal(d2, d3)
        s2, s3 = state_of(on.batch), state_of(tb)
        for f in s2:
            np.testing.assert_array_equal(s2[f], s3[f])
        twin.close()
    off.close(); on.close()


# ---- step_act and dm_batch_rollout with a policy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed,pipeline", [(False, 1), (True, 1), (True, 2)])
def test_step_act_and_rollout_are_step_then_terminate_then_act(packed, pipeline):
    n, Tn = 48, 4
    idx, q, v = states(n, seed=9)
    pol, W = fused_policy()
    a0 = np.random.RandomState(3).randn(n, 28) * 0.9
    results = []
    for how in ("reference", "step_act", "rollout"):
        env = make(n, fall="deepmimic", limit=3, autoreset="rsi", packed=packed, pipeline=pipeline, step_queue=8 if packed else 0)
        b = env.batch
        start(b, idx, q, v)
        ac, ob, rew, dn, vp = horizon_rows(Tn, n, a0=a0)
        if how == "rollout":
            b.rollout(ac, (ob, rew, dn), 1, W, vp, True, pol._seed, 7)
        for t in range(Tn if how != "rollout" else 0):
            if how == "step_act":
                b.step_act(ac[t], 1, (ob[t], rew[t], dn[t]), W, ac[t + 1], vp[t], True, pol._seed, 7 + t)
            else:
                b.step(ac[t], 1, (ob[t], rew[t], dn[t])); b.join()
                pol._counter = 7 + t - 1
                pol.act(True, ob[t], out=ac[t + 1], vpred_out=vp[t])
        b.join(); b.sync()
        assert b.queue_stats() == (0, 0, 0)                          # no horizon launch, nothing queued
        results.append([x.cpu().numpy() for x in (ac, ob, rew, dn, vp)] + [b.get(A.F_DONE_REASON), b.get(A.F_EPISODE_STEPS), b.get(A.F_QPOS)])
        env.close()
    ref = results[0]
    assert ref[3].sum() >= 4 and ref[3][0].sum() < n                 # some episodes ended, by no means all
    for got in results[1:]:
        for x, y in zip(got, ref):
            np.testing.assert_array_equal(x, y)


# ---- the time limit ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_time_limit_from_a_standing_state(packed):
    n = 48
    env = make(n, limit=3, packed=packed)
    b = env.batch
    b.reset(mode=2, hard=1)
    a = np.zeros((n, 28))
    trace = []
    for t in range(1, 8):
        _o, r, d = step_numpy(b, a)
        assert (r == 1.0).all()
        assert (d != 0).all() == (t in (3, 6)) and (d != 0).any() == (t in (3, 6))
        np.testing.assert_array_equal(b.get(A.F_DONE_REASON), np.full(n, T.DONE_TIME_LIMIT if t in (3, 6) else 0))
        trace.append(int(b.get(A.F_EPISODE_STEPS)[0]))
        assert (b.get(A.F_EPISODE_STEPS) == trace[-1]).all()
    assert trace == [1, 2, 0, 1, 2, 0, 1]
    b.set(A.F_EPISODE_STEPS, np.full(n, 2, dtype=np.int32))
    mask = (np.arange(n) % 2).astype(np.uint8)
    b.reset(mode=2, hard=1, mask=mask)                               # dm_batch_reset starts the masked envs' counters again
    np.testing.assert_array_equal(b.get(A.F_EPISODE_STEPS), np.where(mask, 0, 2))
    b.set_option(A.OPT_MAX_EPISODE_STEPS, 1)
    for t in range(3):
        _o, _r, d = step_numpy(b, a)
        assert (d != 0).all() and (b.get(A.F_DONE_REASON) == T.DONE_TIME_LIMIT).all() and not b.get(A.F_EPISODE_STEPS).any()
    env.close()


# ---- closed loop --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", ["walk", "cartwheel"])
def test_closed_loop_invariants_under_random_actions(clip):
    """64 closed-loop steps of 64 envs under N(0, 0.9^2) actions, the "deepmimic" set, auto-reset by RSI.  The invariants hold at every step on both
    clips.  The count of fall terminations is asserted on cartwheel, whose reference plants the hands while the centre of mass is high (13 of its 164
    frames): measured on an MI355X 47 fall terminations and 224 by the step's own rule.  On walk the centre of mass leaves the step's band before any
    body but a foot reaches the floor: measured 0 fall terminations against 140 by the step's own rule (and 0 or 1 in eleven other walk
    configurations: imitation reward, 4 substeps, actions of scale 3, PD-target actions), so there the count is printed, not asserted."""
    n, steps = 64, 64
    cm = H.compiled_model()
    env = DPVecEnv(n, motion=clip, autoreset="rsi", seed=SEED, fall_contact_bodies="deepmimic")
    b = env.batch
    env.reset("rsi")
    rng = np.random.RandomState(0)
    since = np.zeros(n, dtype=np.int64)
    falls = other = 0
    gm = geom_mask()
    for t in range(steps):
        _o, _r, d, _i = env.step(rng.randn(n, 28) * 0.9)
        d = np.asarray(d) != 0
        reason = env.done_reason()
        np.testing.assert_array_equal(reason != 0, d)
        assert not (reason & T.DONE_TIME_LIMIT).any() and not ((reason & T.DONE_STEP != 0) & (reason & T.DONE_FALL != 0)).any()
        live = ~d                                                    # (with auto-reset the state of an env that ended is already its fresh episode's)
        touch = FN.floor_masks(cm, b.get(A.F_QPOS)[live])
        assert not (touch & gm).any(), "a live environment touches the floor with a fall body at step %d" % t
        since = np.where(d, 0, since + 1)
        np.testing.assert_array_equal(b.get(A.F_EPISODE_STEPS), since)
        falls += int(((reason & T.DONE_FALL) != 0).sum()); other += int((reason == T.DONE_STEP).sum())
    print("closed loop on %s: %d fall terminations, %d by the step's own rule, over %d steps of %d envs" % (clip, falls, other, steps, n))
    if clip == "cartwheel":
        assert falls >= n // 2
    env.close()


# ---- a floor clip -------------------------------------------------------------------------------------------------------------------------------
def test_crawl_clip_reference_poses_against_the_two_sets():
    """Crawl's reference poses touch the floor with hands, knees and feet: the "crawl" set (root, chest, neck) flags none of them, the "deepmimic" set
    those the restatement names.  Through a step the clip's COM height (0.16 .. 0.31 m) still ends every episode by the step's own rule, which the
    termination launch records and does not second-guess."""
    n = 48
    cm = H.compiled_model()
    env = DPVecEnv(n, motion="crawl", autoreset="rsi", seed=SEED, fall_contact_bodies="crawl")
    b = env.batch
    env.reset("rsi")
    q = b.get(A.F_QPOS)
    touch = b.floor_contacts()
    np.testing.assert_array_equal(touch, FN.floor_masks(cm, q))
    assert np.count_nonzero(touch) >= n // 4                            # poses on the floor (the others hover just above it) ...
    assert not (touch & geom_mask(T.fall_body_mask("crawl"))).any()     # ... with none of root, chest, neck
    hit = (touch & geom_mask()) != 0
    frames = H.mocap("crawl").data_config
    assert 0 < hit.sum() and abs(hit.mean() - ((FN.floor_masks(cm, frames) & geom_mask()) != 0).mean()) < 0.25
    _o, _r, d, _i = env.step(np.zeros((n, 28)))
    reason = env.done_reason()
    assert not (reason & T.DONE_FALL).any() and (reason == T.DONE_STEP).all() and np.asarray(d).all()
    env.close()


# ---- facades --------------------------------------------------------------------------------------------------------------------------------------
def test_vec_env_kwargs_and_deepmimic_rows_of_terminated_envs():
    n = 48
    cm = H.compiled_model()
    env = DPVecEnv(n, motion="walk", reward="imitation", autoreset="rsi", seed=SEED, obs_mode="deepmimic", fall_contact_bodies=["root", "chest", 3], max_episode_steps=2)
    b = env.batch
    assert b.options[A.OPT_FALL_BODIES] == 0b1110 == env.fall_body_mask and b.options[A.OPT_MAX_EPISODE_STEPS] == 2 == env.max_episode_steps
    env.reset("rsi")
    a = np.zeros((n, 28))
    obs, _r, d, _i = env.step(a)
    assert not np.asarray(d).any() and obs.shape == (n, A.NSTATE)
    ep = b.get(A.F_EPISODE)
    obs, _r, d, _i = env.step(a)
    assert np.asarray(d).all() and (env.done_reason() & T.DONE_TIME_LIMIT).all()
    np.testing.assert_array_equal(b.get(A.F_EPISODE), ep + 1)
    q, v = b.get(A.F_QPOS), b.get(A.F_QVEL)
    fi = b.get(A.F_FRAME_IDX)
    mc = H.mocap("walk")
    np.testing.assert_array_equal(q, mc.data_config[fi])              # the fresh episodes' states ...
    ref = SN.batch_features(cm, q, v, [SN.phase_of(3, k, k, b.n_frames) for k in fi])
    assert max(H.rel_err(obs[e], ref[e]) for e in range(n)) < 1e-9   # ... and their features
    out = torch.zeros(n, dtype=torch.int32, device=DEV)
    assert env.done_reason(out) is out and (out.cpu().numpy() == env.done_reason()).all()
    env.close()


def test_dp_env_kwargs_and_early_termination():
    env = DPEnv(motion="walk", fall_contact_bodies="deepmimic", max_episode_steps=3)
    assert env.early_termination() is False and not env.is_done()
    dones = [env.step(np.zeros(28))[2] for _ in range(3)]
    assert dones == [False, False, True]
    q = env.sim.data.qpos.copy(); q[2] = 0.3                          # the root sphere in the floor, the COM rule aside
    env.set_state(q, np.zeros(34))
    assert env.early_termination() is True
    _o, _r, done, _i = env.step(np.zeros(28))
    assert done
    plain = DPEnv(motion="walk")
    plain.set_state(q, np.zeros(34))
    assert plain.early_termination() is False
    env.close(); plain.close()


def test_training_tool_closes_episodes_at_the_limit(tmp_path):
    import json
    out = str(tmp_path / "trpo.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_trpo.py"), "--envs", "64", "--iters", "2", "--fall-contact", "deepmimic",
                        "--max-episode-steps", "50", "--out", out], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    hist = json.load(open(out))["history"]
    print([(h["EpLenMean"], h["EpLenMeanIter"], h["EpThisIter"]) for h in hist])
    assert len(hist) == 2 and all(h["EpThisIter"] >= 64 and 0 < h["EpLenMean"] <= 50 and 0 < h["EpLenMeanIter"] <= 50 for h in hist), hist


# ---- defaults -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True])
def test_options_at_zero_change_nothing(packed):
    n = 48 if not packed else 66
    idx, q, v, _ws, _c = H.varied_states(n, seed=13)
    rng = np.random.RandomState(2)
    acts = rng.randn(16, n, 28) * 0.9
    runs = []
    for touch in (False, True):
        env = make(n, autoreset="rsi", packed=packed)
        b = env.batch
        if touch:
            b.set_option(A.OPT_FALL_BODIES, DEEPMIMIC); b.set_option(A.OPT_MAX_EPISODE_STEPS, 5)
            b.set_option(A.OPT_FALL_BODIES, 0); b.set_option(A.OPT_MAX_EPISODE_STEPS, 0)
        start(b, idx, q, v)
        rows = [step_numpy(b, acts[t]) for t in range(16)]
        runs.append((rows, state_of(b), b.get(A.F_EPISODE_STEPS), b.get(A.F_DONE_REASON)))
        env.close()
    for (o0, r0, d0), (o1, r1, d1) in zip(runs[0][0], runs[1][0]):
        np.testing.assert_array_equal(o0, o1); np.testing.assert_array_equal(r0, r1); np.testing.assert_array_equal(d0, d1)
    for f in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][f], runs[1][1][f])
    assert not runs[1][2].any() and not runs[1][3].any()             # with both options off the two fields are not maintained
