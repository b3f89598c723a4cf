"""Multi-clip batches (dm_mocap_create_set): the test set and its references (TEST INFRASTRUCTURE), shared by tests/test_clips_multi.py (wave
testbench) and tests/test_gpu_clips_multi.py (device).

The set.  walk (39 frames, wraps), spinkick (78 frames, another dt) and kick ("Loop: none"); env e imitates clip e % 3.  With N = 10 the first
two waves of the packed kernel hold mixed clips and the last wave has two live slots.  The walk envs 0 and 6 and every kick env start on their
clip's frame F - 3, so that within three steps of reward mode 3 a wrap with cycle == 1 and a clip end (done) occur; the tests assert from the
REFERENCE side that both did.

References.  Nothing is taken from the code under test:
  * the oracle, env by env: an oracle Data stepped with its OWN clip's tables, parameters and dt (Data.env_step, env_step_imitation,
    env_step_v1; action modes 1 and 4 through action_reward_cases.host_ctrl / spd_numpy.env_step), up to and including the env's first done;
  * the twins: three single-clip batches of the same N, seed and env_offset — env e of the multi-clip batch is env e of the twin of clip e % 3;
  * the episode-mode mirror: clip = first c with helpers.device_rng_uniform(seed, genv, ep, 128) < cdf[c], then helpers.device_rsi_frame with that
    clip's length.
"""
import numpy as np

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.clips import ClipSet, clip_cdf
from tests import action_reward_cases as AR
from tests import helpers as H
from tests import spd_numpy as S

NAMES = ("walk", "spinkick", "kick")
N = 10
T_ORACLE = 8
ACTION_SCALE = 0.3
_SETS = {}
_EXPECTED = {}


def clip_set(imitation=True, weights=None, names=NAMES):
    key = (bool(imitation), None if weights is None else tuple(weights), tuple(names))
    if key not in _SETS:
        spec = None
        if imitation:
            from deepmimic_mujoco_amd.imitation import ImitationSpec
            spec = ImitationSpec(H.compiled_model())
        _SETS[key] = ClipSet([H.mocap(c) for c in names], weights, spec)
        _SETS[key].names = list(names)
    return _SETS[key]


def start(n=N, K=len(NAMES)):
    """-> (clip [n], frame [n] local to the clip, qpos [n, 35], qvel [n, 34]): the mocap state of the frame every env starts on"""
    cs = clip_set()
    clip = (np.arange(n) % K).astype(np.int32)
    frame = np.zeros(n, dtype=np.int32)
    for e in range(n):
        F = int(cs.n_frames[clip[e]])
        if NAMES[clip[e]] == "kick" or (NAMES[clip[e]] == "walk" and e % 6 == 0):
            frame[e] = F - 3
        else:
            frame[e] = (5 + 7 * e) % (F - 8)
    q = np.stack([cs.mocaps[clip[e]].data_config[frame[e]] for e in range(n)])
    v = np.stack([cs.mocaps[clip[e]].data_vel[frame[e]] for e in range(n)])
    return clip, frame, q, v


def actions(T, n=N, seed=3):
    return np.random.RandomState(seed).randn(T, n, 28) * ACTION_SCALE


prepare = H.start                    # prepare(b, frame, q, v): zero warm start and time, the states at the clips' frames


def oracle_rows(reward_mode, action_mode, nsub=1, T=T_ORACLE, n=N):
    """The oracle's rows of the set above, each env with its own clip -> dict obs [T, n, 56], reward, done [T, n], cursor, cycle [T, n] (after the
    step), valid [T, n] (up to and including the env's first done), wrapped / ended [n] (reward mode 3: a cycle was counted / the clip ended)."""
    key = (reward_mode, action_mode, nsub, T, n)
    if key in _EXPECTED:
        return _EXPECTED[key]
    from oracle import oracle as O
    cs = clip_set()
    cm, om = H.compiled_model(), H.oracle_model()
    h = AR.timestep()
    kp, kd = AR.golden_gains()
    clip, frame, q, v = start(n)
    acts = actions(T, n)
    r = dict(obs=np.zeros((T, n, 56)), reward=np.zeros((T, n)), done=np.zeros((T, n), dtype=np.uint8), cursor=np.zeros((T, n), dtype=np.int32),
             cycle=np.zeros((T, n), dtype=np.int32), valid=np.zeros((T, n), dtype=bool), wrapped=np.zeros(n, dtype=bool), ended=np.zeros(n, dtype=bool))
    for e in range(n):
        mc = cs.mocaps[clip[e]]
        tab, par = cs.imitation[clip[e]]
        F = mc.data_config.shape[0]
        upd = S.update_interval(float(mc.dt), h, nsub) if reward_mode == 4 else 1
        od = O.Data(om); od.reset(); od.set_state(q[e], v[e])
        init = int(frame[e])
        cur = 0 if reward_mode in (2, 4) else init
        cyc = 0
        for t in range(T):
            a = acts[t, e]
            if action_mode in (0, 1):
                c = a
                if action_mode == 1:
                    k = S.start_frame(reward_mode, cur, init, F, upd)
                    c = AR.host_ctrl(1, a, mc.data_config[k], mc.data_vel[k], od.get("qpos", 40), od.get("qvel", 40), kp, kd)
                if reward_mode <= 2:
                    o, rew, dn, cur = od.env_step(c, nsub, reward_mode, mc.data_config, cur, init)
                elif reward_mode == 3:
                    o, rew, dn, cur, cyc = O.env_step_imitation(om, od, c, nsub, tab, par, cur, cyc)
                else:
                    o, rew, dn, cur = O.env_step_v1(om, od, c, nsub, tab, par, float(mc.dt), cur, init)
            else:
                o, rew, dn, nxt, _c = S.env_step(cm, od, action_mode, a, mc, cur, nsub, h, reward_mode=reward_mode, frame_init=init, imit=(tab, par), cycle=cyc)
                cur, cyc = nxt if reward_mode == 3 else (nxt, cyc)
            r["obs"][t, e] = o; r["reward"][t, e] = rew; r["done"][t, e] = dn; r["cursor"][t, e] = cur; r["cycle"][t, e] = cyc; r["valid"][t, e] = True
            if reward_mode == 3:
                r["wrapped"][e] = r["wrapped"][e] or cyc > 0
                r["ended"][e] = r["ended"][e] or (dn and par[15] == 0 and cur == F - 1)
            if dn:
                break
    for x in r.values():
        x.setflags(write=False)
    _EXPECTED[key] = r
    return r


def check_oracle(b, reward_mode, action_mode, nsub=1, tol=1e-9):
    """step `b` (a multi-clip batch, device or testbench, options set, autoreset off) through the oracle case and compare env by env"""
    exp = oracle_rows(reward_mode, action_mode, nsub)
    T, n = exp["done"].shape
    clip, frame, q, v = start(n)
    assert np.array_equal(b.get(A.F_CLIP), clip)
    prepare(b, frame, q, v)
    acts = actions(T, n)
    worst = 0.0
    for t in range(T):
        obs, rew, done = b.step(acts[t], nsub)[:3]
        cur, cyc = b.get(A.F_FRAME_IDX), b.get(A.F_CYCLE)
        for e in range(n):
            if not exp["valid"][t, e]:
                continue
            worst = max(worst, H.rel_err(obs[e], exp["obs"][t, e]), abs(rew[e] - exp["reward"][t, e]) / max(1.0, abs(exp["reward"][t, e])))
            assert bool(done[e]) == bool(exp["done"][t, e]), ("done", t, e)
            assert cur[e] == exp["cursor"][t, e] and cyc[e] == exp["cycle"][t, e], ("cursor / cycle", t, e, cur[e], exp["cursor"][t, e], cyc[e], exp["cycle"][t, e])
    assert np.array_equal(b.get(A.F_FRAME_INIT), frame)
    print("reward mode %d, action mode %d: worst relative error %.3e" % (reward_mode, action_mode, worst))
    assert worst < tol, worst
    if reward_mode == 3:      # from the reference side: a wrap that counted a cycle, and a clip end
        assert exp["wrapped"][clip == 0].any() and exp["ended"][clip == 2].all() and not exp["ended"][clip != 2].any()
    return worst


TWIN_FIELDS = (A.F_QPOS, A.F_QVEL, A.F_FRAME_IDX, A.F_FRAME_INIT, A.F_CYCLE, A.F_EPISODE, A.F_TIME)


def check_twins(multi, twins, T, nsub=1, exact=True, tol=1e-9, extra_fields=()):
    """env e of `multi` against env e of twins[e % K], T steps from the set's start with the set's actions -> done [T, n].  exact: bit for bit;
    otherwise flags, counters and cursors exactly and floats within tol (the packed lean kernel's rule for rows 33..40)."""
    n = multi.n
    K = len(twins)
    clip, frame, q, v = start(n, K)
    cs = clip_set()
    prepare(multi, frame, q, v)
    for k, b in enumerate(twins):
        prepare(b, np.minimum(frame, int(cs.n_frames[k]) - 1), q, v)       # (an env of another clip only needs a frame inside this one)
    acts = actions(T, n, seed=11)
    dones = np.zeros((T, n), dtype=np.uint8)
    sel = [np.nonzero(clip == k)[0] for k in range(K)]

    def same(a, b_, what):
        a, b_ = np.asarray(a), np.asarray(b_)
        if exact or a.dtype.kind in "iub":
            assert np.array_equal(a, b_), what
        else:
            assert H.rel_err(a, b_) < tol, (what, H.rel_err(a, b_))
    for t in range(T):
        o, r, d = multi.step(acts[t], nsub)[:3]
        dones[t] = d
        for k, b in enumerate(twins):
            ok, rk, dk = b.step(acts[t], nsub)[:3]
            same(d[sel[k]], dk[sel[k]], ("done", t, k)); same(o[sel[k]], ok[sel[k]], ("obs", t, k)); same(r[sel[k]], rk[sel[k]], ("reward", t, k))
    for f in TWIN_FIELDS + tuple(extra_fields):
        got = multi.get(f)
        for k, b in enumerate(twins):
            same(got[sel[k]], b.get(f)[sel[k]], ("field", f, k))
    return dones


def episode_mirror(cs, seed, n, resets, env_offset=0, episode0=0):
    """-> (clip [resets, n], frame_init [resets, n]) of clip_mode "episode" after each of `resets` resets that set the frame cursor"""
    clip = np.zeros((resets, n), dtype=np.int32); frame = np.zeros((resets, n), dtype=np.int32)
    for r in range(resets):
        for e in range(n):
            u = H.device_rng_uniform(seed, env_offset + e, episode0 + r, 128)
            c = 0
            while c < len(cs) - 1 and not (u < cs.cdf[c]):
                c += 1
            clip[r, e] = c
            frame[r, e] = H.device_rsi_frame(seed, env_offset + e, episode0 + r, int(cs.n_frames[c]))
    return clip, frame


EPISODE_SEED = 5        # with weights (1, 2, 1), 12 envs and 3 resets the mirror draws every clip (test_clips_multi.py checks it)
