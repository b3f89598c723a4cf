"""Multi-clip batches on the device (dm_mocap_create_set; kernels_clips.hip, kernels_packed_clips.hip): every env of a mixed batch against the oracle
stepped with its own clip, against single-clip twins bit for bit, the episode-mode draw against its host mirror, sharding, and the views.
tests/clips_cases.py has the test set (walk / spinkick / kick, N = 10, env e on clip e % 3) and the references; tests/test_clips_multi.py runs
the same checks on the wave testbench.

Bars.  Oracle: the suite's 1e-9 relative on observation and reward; done, frame_idx, frame_init and cycle exactly.  Twins: bit for bit on
DM_OPT_PACKED 0 and 2 and in the float32 library on 0 — the clip forms evaluate the same source expressions on the same operands, and the packed
forms do not depend on wave neighbours; on DM_OPT_PACKED 1 flags, counters and cursors exactly and floats within 1e-9, the header's rule for rows 33..40."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch, DPVecEnv
from deepmimic_mujoco_amd.termination import fall_body_mask
from tests import clips_cases as CC
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _multi(cs, n, packed=0, reward_mode=3, action_mode=0, autoreset=0, seed=0, env_offset=0, clip_mode=0, dtype=64, term=False):
    b = Batch(H.compiled_model(), None, None, n, device=0, dtype=dtype, clips=cs)
    _options(b, packed, reward_mode, action_mode, autoreset, seed, env_offset, term)
    b.set_option(A.OPT_CLIP_MODE, clip_mode)
    return b


def _twin(cs, k, n, packed=0, reward_mode=3, action_mode=0, autoreset=0, seed=0, env_offset=0, dtype=64, term=False):
    m = cs.mocaps[k]
    b = Batch(H.compiled_model(), m.data_config, m.data_vel, n, device=0, mocap_dt=float(m.dt), imitation=cs.imitation[k], dtype=dtype)
    _options(b, packed, reward_mode, action_mode, autoreset, seed, env_offset, term)
    return b


def _options(b, packed, reward_mode, action_mode, autoreset, seed, env_offset, term):
    b.set_option(A.OPT_REWARD_MODE, reward_mode); b.set_option(A.OPT_ACTION_MODE, action_mode); b.set_option(A.OPT_AUTORESET, autoreset)
    b.set_option(A.OPT_SEED, seed); b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_ENV_OFFSET, env_offset)
    if term:
        b.set_option(A.OPT_FALL_BODIES, fall_body_mask("deepmimic")); b.set_option(A.OPT_MAX_EPISODE_STEPS, 5)


# ---- 1. the oracle, env by env ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("action_mode", [0, 1, 4])
@pytest.mark.parametrize("reward_mode", [1, 2, 3, 4])
def test_oracle_env_by_env(reward_mode, action_mode, packed):
    b = _multi(CC.clip_set(), CC.N, packed, reward_mode, action_mode)
    CC.check_oracle(b, reward_mode, action_mode)
    b.close()


# ---- 2. twins ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("autoreset", [1, 2], ids=["rsi", "init"])
@pytest.mark.parametrize("packed,dtype,term", [(0, 64, False), (2, 64, False), (1, 64, False), (0, 32, False), (0, 64, True), (2, 64, True)],
                         ids=["one-env", "packed-ext", "packed-lean", "one-env-f32", "one-env-term", "packed-ext-term"])
def test_twins(packed, dtype, term, autoreset):
    cs = CC.clip_set()
    multi = _multi(cs, CC.N, packed, 3, autoreset=autoreset, seed=7, env_offset=3, dtype=dtype, term=term)
    multi.set(A.F_CLIP, np.arange(CC.N, dtype=np.int32) % 3)            # (env_offset 3 dealt (3 + e) % 3 — the same here; the write is exercised)
    twins = [_twin(cs, k, CC.N, packed, 3, autoreset=autoreset, seed=7, env_offset=3, dtype=dtype, term=term) for k in range(3)]
    extra = (A.F_EPISODE_STEPS, A.F_DONE_REASON) if term else ()
    dones = CC.check_twins(multi, twins, 48, exact=packed != 1, extra_fields=extra)
    per_clip = [bool(dones[:, k::3].any()) for k in range(3)]
    assert per_clip[2] and sum(per_clip) >= 2, per_clip                  # auto-resets in envs of at least two clips; kick guarantees one
    assert np.array_equal(multi.get(A.F_CLIP), np.arange(CC.N) % 3)      # "fixed": a reset keeps the clip
    for b in [multi] + twins:
        b.close()


# ---- 3. episode mode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [0, 1])
def test_episode_mode_against_host_mirror(packed):
    cs = CC.clip_set(weights=(1, 2, 1))
    n, seed = 12, CC.EPISODE_SEED
    b = _multi(cs, n, packed, 3, autoreset=1, seed=seed, clip_mode=1)
    clip, frame = CC.episode_mirror(cs, seed, n, 3)
    assert set(clip.ravel().tolist()) == {0, 1, 2}
    for r in range(3):
        b.reset(0, 1)
        assert np.array_equal(b.get(A.F_CLIP), clip[r]) and np.array_equal(b.get(A.F_FRAME_INIT), frame[r]) and np.array_equal(b.get(A.F_FRAME_IDX), frame[r])
        q = b.get(A.F_QPOS)
        for e in range(n):
            assert np.array_equal(q[e], cs.mocaps[clip[r, e]].data_config[frame[r, e]])
    # the in-kernel auto-reset: envs dropped below the COM band start episode 3 on the mirror's clip and frame
    q = b.get(A.F_QPOS); q[::2, 2] = 0.3
    b.set_state(q, b.get(A.F_QVEL))
    _o, _r, d = b.step(np.zeros((n, 28)))
    c3, f3 = CC.episode_mirror(cs, seed, n, 1, episode0=3)
    assert d[::2].all()
    got_c, got_f = b.get(A.F_CLIP), b.get(A.F_FRAME_INIT)
    assert np.array_equal(got_c[d != 0], c3[0][d != 0]) and np.array_equal(got_f[d != 0], f3[0][d != 0])
    assert np.array_equal(got_c[d == 0], clip[2][d == 0])
    b.close()
    # the termination launch's reset draws as well: a time limit of 1 ends every episode at its first step
    b = _multi(cs, n, packed, 3, autoreset=1, seed=seed, clip_mode=1)
    b.set_option(A.OPT_MAX_EPISODE_STEPS, 1)
    b.reset(0, 1)
    _o, _r, d = b.step(np.zeros((n, 28)))
    c1, f1 = CC.episode_mirror(cs, seed, n, 1, episode0=1)
    assert d.all() and np.array_equal(b.get(A.F_CLIP), c1[0]) and np.array_equal(b.get(A.F_FRAME_INIT), f1[0])
    b.close()
    b = _multi(CC.clip_set(weights=(0, 1, 0)), n, packed, 3, seed=seed, clip_mode=1)
    b.reset(0, 1)
    assert (b.get(A.F_CLIP) == 1).all()
    b.close()


# ---- 4. sharding -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [0, 2])
def test_two_shards_equal_one_batch(packed):
    cs = CC.clip_set(weights=(1, 2, 1))
    seed = 21
    whole = _multi(cs, 12, packed, 3, autoreset=1, seed=seed, clip_mode=1)
    parts = [_multi(cs, 6, packed, 3, autoreset=1, seed=seed, env_offset=off, clip_mode=1) for off in (0, 6)]
    assert np.array_equal(np.concatenate([p.get(A.F_CLIP) for p in parts]), whole.get(A.F_CLIP))      # the default assignment follows the global env id
    for b in [whole] + parts:
        b.reset(0, 1)
    acts = CC.actions(16, 12, seed=4)
    for t in range(16):
        o, r, d = whole.step(acts[t])
        for k, p in enumerate(parts):
            sl = slice(6 * k, 6 * k + 6)
            ok, rk, dk = p.step(acts[t, sl])
            assert np.array_equal(o[sl], ok) and np.array_equal(r[sl], rk) and np.array_equal(d[sl], dk), t
    for f in CC.TWIN_FIELDS + (A.F_CLIP,):
        assert np.array_equal(np.concatenate([p.get(f) for p in parts]), whole.get(f)), f
    for b in [whole] + parts:
        b.close()


# ---- 5. views, validation, horizon and queue -----------------------------------------------------------------------------------------------------
def test_views_and_validation():
    cs = CC.clip_set()
    n = CC.N
    clip, frame, q, v = CC.start(n)
    multi = _multi(cs, n, 0, 3)
    twins = [_twin(cs, k, n, 0, 3) for k in range(3)]
    CC.prepare(multi, frame, q, v)
    for k, b in enumerate(twins):
        CC.prepare(b, np.minimum(frame, int(cs.n_frames[k]) - 1), q, v)
    a = CC.actions(1, n)[0]
    for b in [multi] + twins:
        b.step(a)
    feats, terms = multi.state_features(), multi.imitation_terms()
    ids = np.array([4, 2, 9], dtype=np.int32)
    terms_ids = multi.imitation_terms(env_ids=ids)
    for e in range(n):
        tw = twins[clip[e]]
        one = np.array([e], dtype=np.int32)
        assert np.array_equal(feats[e], tw.state_features(env_ids=one)[0]) and np.array_equal(terms[e], tw.imitation_terms(env_ids=one)[0])
    assert np.array_equal(terms_ids, terms[ids])
    # the phase runs over the env's own clip length
    from deepmimic_mujoco_amd import state_features as SF
    cur = multi.get(A.F_FRAME_IDX)
    assert np.allclose(feats[:, SF.O_PHASE], cur / cs.n_frames[clip].astype(np.float64), rtol=0, atol=1e-15)
    # explicit states: frame i is local to the clip of env i — frame 60 exists in spinkick (78 frames), not in walk (39) or kick (47)
    fr = np.minimum(60, cs.n_frames[clip] - 1).astype(np.int32)
    ex = multi.imitation_terms(qpos=q, qvel=v, frame=fr)
    for e in range(n):
        tw = twins[clip[e]]
        assert np.array_equal(ex[e], tw.imitation_terms(qpos=q[e:e + 1], qvel=v[e:e + 1], frame=fr[e:e + 1])[0])
    bad = fr.copy(); bad[0] = 60
    with pytest.raises(A.DmenvError) as ei:
        multi.imitation_terms(qpos=q, qvel=v, frame=bad)
    assert "-1" in str(ei.value) and "clip" in str(ei.value)
    ok = fr.copy(); ok[1] = 60
    multi.imitation_terms(qpos=q, qvel=v, frame=ok)
    with pytest.raises(A.DmenvError):
        multi.set_state(q, v, frame_idx=bad)
    multi.set_state(q, v, frame_idx=ok)
    # DM_F_CLIP validates its range; a profiling launch is unsupported
    with pytest.raises(A.DmenvError):
        multi.set(A.F_CLIP, np.full(n, 3, dtype=np.int32))
    with pytest.raises(A.DmenvError):
        multi.set(A.F_CLIP, torch.full((n,), -1, dtype=torch.int32, device=DEV))
    multi.set_option(101, 1)
    with pytest.raises(A.DmenvError) as ei:
        multi.step(a)
    assert "-4" in str(ei.value)
    multi.set_option(101, 0)
    # a set whose shared parameters differ is refused
    from deepmimic_mujoco_amd.clips import ClipSet
    odd = ClipSet([H.mocap("walk"), H.mocap("kick")], None, None)
    par = np.array(cs.imitation[2][1]); par[3] += 0.5
    odd.imitation = [cs.imitation[0], (cs.imitation[2][0], par)]
    with pytest.raises(A.DmenvError) as ei:
        Batch(H.compiled_model(), None, None, 4, device=0, clips=odd)
    assert "-1" in str(ei.value)
    for b in [multi] + twins:
        b.close()


def test_set_of_one_is_the_clip_alone():
    cs1 = CC.clip_set(names=("spinkick",))
    m = cs1.mocaps[0]
    a = Batch(H.compiled_model(), None, None, 6, device=0, clips=cs1)
    b = Batch(H.compiled_model(), m.data_config, m.data_vel, 6, device=0, mocap_dt=float(m.dt), imitation=cs1.imitation[0])
    for x in (a, b):
        _options(x, 1, 3, 0, 1, 9, 0, False)
        x.reset(0, 1)
    acts = CC.actions(6, 6)
    for t in range(6):
        ra, rb = a.step(acts[t]), b.step(acts[t])
        assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
    assert (a.get(A.F_CLIP) == 0).all() and np.array_equal(a.get(A.F_FRAME_IDX), b.get(A.F_FRAME_IDX))
    a.close(); b.close()


@pytest.mark.parametrize("form", ["rollout", "queue"])
def test_horizon_and_queue_give_what_step_launches_give(form):
    cs = CC.clip_set()
    n, T = CC.N, 6
    clip, frame, q, v = CC.start(n)
    acts = CC.actions(T, n)
    ref = _multi(cs, n, 1, 3, autoreset=1, seed=2)
    CC.prepare(ref, frame, q, v)
    exp = [ref.step(acts[t]) for t in range(T)]
    b = _multi(cs, n, 1, 3, autoreset=1, seed=2)
    b.set_option(106, 1)                      # ask for the one-launch horizon: a multi-clip batch still issues step launches
    CC.prepare(b, frame, q, v)
    a_d = torch.zeros((T + 1, n, 28), dtype=torch.float64, device=DEV); a_d[:T] = torch.as_tensor(acts, device=DEV)
    out = (torch.zeros((T, n, 56), dtype=torch.float64, device=DEV), torch.zeros((T, n), dtype=torch.float64, device=DEV), torch.zeros((T, n), dtype=torch.uint8, device=DEV))
    if form == "rollout":
        b.rollout(a_d, out)
    else:
        b.set_option(A.OPT_STEP_QUEUE, 4)
        for t in range(T):
            b.step(a_d[t], 1, (out[0][t], out[1][t], out[2][t]))
        b.join()
        assert b.queue_stats()[0] == 0        # nothing was queued
    b.sync()
    for t in range(T):
        for k in range(3):
            assert np.array_equal(out[k][t].cpu().numpy(), exp[t][k]), (t, k)
    for f in CC.TWIN_FIELDS:
        assert np.array_equal(b.get(f), ref.get(f)), f
    ref.close(); b.close()


def test_vec_env_motion_list():
    env = DPVecEnv(9, motion=list(CC.NAMES), reward="imitation", autoreset="rsi", seed=CC.EPISODE_SEED, clip_weights=(1, 2, 1), clip_mode="episode", packed=False)
    assert len(env.clip_set) == 3 and np.array_equal(env.clip_ids(), np.arange(9) % 3)
    env.reset()
    clip, frame = CC.episode_mirror(env.clip_set, CC.EPISODE_SEED, 9, 1)
    assert np.array_equal(env.clip_ids(), clip[0]) and np.array_equal(env.batch.get(A.F_FRAME_INIT), frame[0])
    env.set_clip_ids(np.zeros(9, dtype=np.int32))
    # the cursors are left alone, except that one beyond the new clip (walk: 39 frames) is held on its last frame
    assert (env.clip_ids() == 0).all() and np.array_equal(env.batch.get(A.F_FRAME_INIT), np.minimum(frame[0], 38))
    assert (frame[0] > 38).any() and (frame[0] < 38).any()
    with pytest.raises(ValueError):
        DPVecEnv(4, motion="walk", clip_weights=(1, 2))
    env.close()


def test_clip_write_holds_the_cursors_inside_the_new_clip():
    """dm_batch_set(DM_F_CLIP) leaves the cursors alone, except that one naming a row beyond the new clip becomes that clip's last frame: a step taken before
    the reset the contract asks for stays inside the clip's rows (kick is the LAST clip of the set: frame 70 of spinkick would read past the tables' end)"""
    cs = CC.clip_set()
    n = 6
    for reward_mode in (1, 2):
        b = _multi(cs, n, 0, reward_mode, action_mode=1)
        b.set(A.F_CLIP, np.ones(n, dtype=np.int32))
        fr = np.array([70, 70, 45, 46, 47, 10], dtype=np.int32)
        m = cs.mocaps[1]
        b.set_state(m.data_config[fr], m.data_vel[fr], frame_idx=fr)
        b.set(A.F_CLIP, np.array([2, 0, 2, 2, 2, 1], dtype=np.int32))          # kick has 47 frames, walk 39
        want = np.array([46, 38, 45, 46, 46, 10], dtype=np.int32)
        assert np.array_equal(b.get(A.F_FRAME_INIT), want)
        assert np.array_equal(b.get(A.F_FRAME_IDX), np.zeros(n, dtype=np.int32) if reward_mode == 2 else want)
        o, r, d = b.step(np.zeros((n, 28)))
        assert np.isfinite(o).all() and np.isfinite(r).all()
        b.close()


def test_time_limit_bootstrap_takes_the_phase_over_the_envs_clip():
    """SegmentCollector(bootstrap_time_limit=True) with the 171-wide observation on a list of motions: the phase of a truncated state runs over the length
    of the env's own clip (clip_mode "fixed"); with clip_mode "episode" the clip has been redrawn when the log is read, and the combination is refused"""
    from deepmimic_mujoco_amd import MlpPolicy
    from deepmimic_mujoco_amd.rollout import SegmentCollector
    from deepmimic_mujoco_amd.state_features import phase_of
    n, T, M = 9, 7, 3
    kw = dict(motion=list(CC.NAMES), reward="imitation", autoreset="init", seed=3, obs_mode="deepmimic", max_episode_steps=M, packed=False, frame_skip=1)
    env = DPVecEnv(n, **kw)
    pi = MlpPolicy(ob_dim=env.observation_space.shape[0], device=DEV, seed=3); pi.seed(4)
    c = SegmentCollector(pi, env, T, bootstrap_time_limit=True)
    c.launch()
    seg = c.collect()
    count, ridx, rq, rv = env.batch.truncations(clear=False, device=False)
    count = int(count[0]); ridx, rq, rv = ridx[:count], rq[:count], rv[:count]
    assert count >= n                                                    # every env meets the limit at row 2
    F = np.asarray(env.clip_set.n_frames)[np.arange(n) % 3][ridx[:, 0]]
    assert len(set(F.tolist())) == 3
    phase = np.array([phase_of(3, int(ridx[i, 2]), int(ridx[i, 3]), int(F[i])) for i in range(count)], dtype=np.float64)
    ob = env.batch.state_features(qpos=rq, qvel=rv, phase=phase)
    with torch.no_grad():
        want = pi.forward_value(torch.as_tensor(ob, device=DEV)).cpu().numpy()
    got = seg["vboot"].cpu().numpy()[ridx[:, 1], ridx[:, 0]]
    assert np.allclose(got, want, rtol=1e-4, atol=1e-5)
    # the phase over the concatenated tables' length is another number (what the batch's total row count would give)
    wrong = np.array([phase_of(3, int(ridx[i, 2]), int(ridx[i, 3]), int(env.batch.n_frames)) for i in range(count)])
    assert np.abs(wrong - phase).max() > 0.01
    env.close()
    env = DPVecEnv(n, clip_mode="episode", **kw)
    with pytest.raises(ValueError):
        SegmentCollector(pi, env, T, bootstrap_time_limit=True)
    env.close()
    env = DPVecEnv(n, clip_mode="episode", **dict(kw, obs_mode="dp_env_v3"))      # the 56-wide observation has no phase: accepted
    SegmentCollector(MlpPolicy(device=DEV, seed=3), env, T, bootstrap_time_limit=True)
    env.close()
