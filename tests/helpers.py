import os

import numpy as np

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.humanoid import humanoid_spec
from deepmimic_mujoco_amd.mocap import MocapDM
from deepmimic_mujoco_amd.model import CompiledModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CM = None
_MOCAP = {}


def compiled_model():
    global _CM
    if _CM is None:
        _CM = CompiledModel(humanoid_spec())
    return _CM


def mocap(clip="walk"):
    if clip not in _MOCAP:
        m = MocapDM(); m.load_mocap(clip); _MOCAP[clip] = m
    return _MOCAP[clip]


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    if a.size == 0 and b.size == 0:
        return 0.0
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def varied_states(n, seed=0, clip="walk"):
    """Seeded states around mocap frames: exact frames, perturbed poses (limits violated, feet in the floor), spins."""
    mc = mocap(clip)
    F = mc.data_config.shape[0]
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, F, size=n).astype(np.int32)
    q = mc.data_config[idx].copy(); v = mc.data_vel[idx].copy()
    for e in range(n):
        kind = e % 4
        if kind == 1:
            q[e, 7:] += 0.3 * rng.randn(28); v[e] += rng.randn(34)
        elif kind == 2:
            q[e, 7:] += 0.6 * rng.randn(28); q[e, 2] -= 0.08 * rng.rand(); q[e, 3:7] += 0.1 * rng.randn(4); v[e] += 2 * rng.randn(34)
        elif kind == 3:
            q[e, 2] -= 0.3 + 0.3 * rng.rand(); q[e, 3:7] = rng.randn(4); q[e, 7:] = rng.uniform(-1, 1, 28); v[e] = 3 * rng.randn(34)
    ws = rng.randn(n, 34) * 3
    ctrl = rng.randn(n, 28) * 0.9
    return idx, q, v, ws, ctrl


# ---- a batch's state: the pieces every test of a batch shares (tests/gpu_batch.py has those that need torch) --------------------------------
STATE = (A.F_QPOS, A.F_QVEL, A.F_QACC_WARMSTART, A.F_TIME, A.F_FRAME_IDX, A.F_FRAME_INIT, A.F_CYCLE, A.F_EPISODE)
TERM_FIELDS = (A.F_EPISODE_STEPS, A.F_DONE_REASON)


def start(b, idx, q, v, ws=None, steps0=None):
    """the batch into a known state: warm start `ws` (zeros), time 0, (q, v) at the mocap frames `idx`, the episodes' step counters at `steps0`"""
    b.set(A.F_QACC_WARMSTART, np.zeros((b.n, 34)) if ws is None else ws); b.set(A.F_TIME, np.zeros(b.n))
    b.set_state(q, v, frame_idx=idx)
    if steps0 is not None:
        b.set(A.F_EPISODE_STEPS, steps0)


def state_of(b, fields=STATE):
    return {f: b.get(f) for f in fields}


def put_state(b, s, ep_steps=None):
    """the batch into the state `s` (state_of of another batch)"""
    b.set(A.F_QACC_WARMSTART, s[A.F_QACC_WARMSTART]); b.set(A.F_TIME, s[A.F_TIME])
    b.set_state(s[A.F_QPOS], s[A.F_QVEL], frame_idx=s[A.F_FRAME_IDX])
    for f in (A.F_FRAME_IDX, A.F_FRAME_INIT, A.F_CYCLE, A.F_EPISODE):
        b.set(f, s[f])
    if ep_steps is not None:
        b.set(A.F_EPISODE_STEPS, ep_steps)


def _first_difference(x, y):
    """where two arrays of one size start to differ: the index, by bytes (a NaN's pattern and the sign of a zero count)"""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    if x.size != y.size or x.dtype != y.dtype:
        return "shape %s %s against %s %s" % (x.shape, x.dtype, y.shape, y.dtype)
    bad = np.nonzero((x.reshape(x.size, 1).view(np.uint8) != y.reshape(y.size, 1).view(np.uint8)).any(1))[0]
    return "%d of %d values differ, first at %s" % (len(bad), x.size, list(np.unravel_index(bad[0], y.shape or (1,))))


def assert_bits(got, ref, what=""):
    """two dicts of arrays, bit for bit (`.tobytes()`); a failure names the key and the first differing index: (step, env, ...) of a row array,
    (env, ...) of a state field"""
    assert got.keys() == ref.keys(), (what, sorted(map(str, got)), sorted(map(str, ref)))
    for k in ref:
        if np.asarray(got[k]).tobytes() != np.asarray(ref[k]).tobytes():
            raise AssertionError("%s %s: %s" % (what, k, _first_difference(got[k], ref[k])))


def assert_bits_or_close(got, ref, tol):
    """integer, bool and uint8 arrays bit for bit; floating arrays finite and within `tol`, relative to max(1, |x|)"""
    assert got.keys() == ref.keys()
    for k in ref:
        if ref[k].dtype.kind in "iub":
            np.testing.assert_array_equal(got[k], ref[k], err_msg=str(k))
        else:
            err = np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))
            assert np.isfinite(got[k]).all() and err.max() <= tol, "%s: %d values differ, by at most %.3e (relative to max(1, |x|))" % (k, (err > 0).sum(), err.max())


def oracle_model(max_efc=63, **opts):
    from oracle import oracle as O
    om = O.Model()
    om.set("max_efc", max_efc)
    for k, val in opts.items():
        om.set(k, val)
    return om


def compare_forward(batch, om, idx, q, v, ws, ctrl, tol=1e-9, failures=None):
    """Stage-by-stage comparison of one forward evaluation per env (debug dump vs oracle).  With `failures` (a list) a mismatching
    env is appended to it as (env, message) and the sweep goes on; without, the first mismatch raises."""
    from oracle import oracle as O
    n = q.shape[0]
    batch.set(A.F_QACC_WARMSTART, ws); batch.set(A.F_CTRL, ctrl)
    batch.set_state(q, v, frame_idx=idx)
    cg_all = batch.get(A.F_CONTACT_GEOMS)
    od = O.Data(om)
    worst = {}

    def one(e):
        od.set("qacc_warmstart", ws[e]); od.set("ctrl", ctrl[e]); od.set_state(q[e], v[e])
        dbg = batch.debug_forward(e)
        nefc, ncon = int(od.get("nefc")[0]), int(od.get("ncon")[0])
        assert dbg["nefc"] == nefc and dbg["ncon"] == ncon, (e, dbg["nefc"], nefc, dbg["ncon"], ncon)
        assert dbg["solver_iter"] == int(od.get("solver_iter")[0]), "PGS sweep count differs for env %d" % e
        ocg = od.get("contact_geom").reshape(-1, 2).astype(np.int32)
        k = min(ncon, A.MAXEFC)
        assert np.array_equal(cg_all[e][:k], ocg[:k]), "contact (geom1, geom2) list differs for env %d" % e
        assert np.all(cg_all[e][k:] == -1)
        J = od.get("efc_J").reshape(-1, 34)[:nefc]
        pairs = [("M", dbg["M"], od.get("M").reshape(34, 34)), ("qfrc_bias", dbg["qfrc_bias"], od.get("qfrc_bias")),
                 ("qacc_smooth", dbg["qacc_smooth"], od.get("qacc_smooth")), ("efc_J", dbg["efc_J"], J),
                 ("efc_pos", dbg["efc_pos"], od.get("efc_pos")[:nefc]), ("efc_R", dbg["efc_R"], od.get("efc_R")[:nefc]),
                 ("efc_aref", dbg["efc_aref"], od.get("efc_aref")[:nefc]), ("efc_b", dbg["efc_b"], od.get("efc_b")[:nefc]),
                 ("efc_force", dbg["efc_force"], od.get("efc_force")[:nefc]), ("qacc", dbg["qacc"], od.get("qacc")),
                 ("xipos", dbg["xipos"], od.get("xipos").reshape(14, 3))]
        errs = {name: rel_err(a, b) for name, a, b in pairs}
        if failures is not None:
            bad = [name for name, _a, _b in pairs if not errs[name] < tol]
            assert not bad, "%s: rel err %.3e (env %d)" % (bad[0], errs[bad[0]], e)
        for name, w in errs.items():
            worst[name] = max(worst.get(name, 0.0), w)

    for e in range(n):
        if failures is None:
            one(e)
        else:
            try:
                one(e)
            except AssertionError as ex:
                failures.append((e, str(ex)))
    if failures is None:
        for name, w in worst.items():
            assert w < tol, "%s: rel err %.3e" % (name, w)
    return worst


def compare_rollout(batch, om, idx, q, v, steps, seed=0, reward_mode=0, n_substeps=1, tol=1e-9, action_scale=0.9, clip="walk"):
    """Lock-step rollout of every env against its own oracle instance; checks obs, reward, done, frame index.
    `clip` must be the clip the batch was created with (its data_config is the oracle's reward table)."""
    from oracle import oracle as O
    n = q.shape[0]
    mc = mocap(clip)
    start(batch, idx, q, v)
    ods = [O.Data(om) for _ in range(n)]
    for e in range(n):
        ods[e].reset(); ods[e].set_state(q[e], v[e])
    # dp_env_v2's cursor counts steps from 0 and adds idx_init at look-up (src/dp_env_v2.py:68-70,128-129); dp_env_v3's starts at the draw
    fidx = np.zeros(n, dtype=np.int64) if reward_mode == 2 else idx.astype(np.int64).copy()
    finit = idx.astype(np.int64).copy()
    rng = np.random.RandomState(seed)
    worst = 0.0
    ndone = 0
    for t in range(steps):
        a = rng.randn(n, 28) * action_scale
        obs, rew, done = batch.step(a, n_substeps)[:3]
        for e in range(n):
            o, r, d, ic = ods[e].env_step(a[e], n_substeps, reward_mode, mc.data_config, int(fidx[e]), int(finit[e]))
            fidx[e] = ic
            worst = max(worst, rel_err(obs[e], o), abs(rew[e] - r) / max(1.0, abs(r)))
            assert bool(done[e]) == d, (t, e)
            ndone += int(d)
        if reward_mode:
            assert np.array_equal(batch.get(A.F_FRAME_IDX), fidx.astype(np.int32))
    assert worst < tol, "rollout rel err %.3e" % worst
    qf = batch.get(A.F_QPOS); wf = batch.get(A.F_QACC_WARMSTART); tf = batch.get(A.F_TIME)
    for e in range(n):
        assert rel_err(qf[e], ods[e].get("qpos")) < tol
        assert rel_err(wf[e], ods[e].get("qacc_warmstart")) < max(tol, 1e-8)
        assert abs(tf[e] - ods[e].get("time")[0]) < 1e-12
    return worst, ndone


def many_row_states(lo, hi, want=4, seed=13, pool=80):
    """Seeded states whose first forward evaluation has lo < nefc <= hi constraint rows (oracle count): exercises the
    overflow strip of the register-tier kernel (columns of A past its register capacity)."""
    from oracle import oracle as O
    om = oracle_model()
    idx, q, v, _ws, _c = varied_states(pool, seed=seed)
    rng = np.random.RandomState(seed)
    for e in range(pool):                       # crouched / lying / half-sunk poses collect many contacts
        if e % 2:
            q[e, 2] = 0.05 + 0.25 * rng.rand(); v[e] *= 0.2
    od = O.Data(om)
    keep = []
    for e in range(pool):
        od.reset(); od.set_state(q[e], v[e])
        ne = int(od.get("nefc")[0])
        if lo < ne <= hi:
            keep.append(e)
        if len(keep) == want:
            break
    assert len(keep) >= min(want, 2), "no states with %d < nefc <= %d in the pool" % (lo, hi)
    k = np.asarray(keep)
    return idx[k], q[k], v[k]


# ---- host mirror of the device's counter-based RNG (csrc/env_step.h: mix64 / rng_uniform) ---------------------------------
_M64 = (1 << 64) - 1


def _mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def device_rng_uniform(seed, genv, episode, k):
    h = _mix64((seed & _M64) ^ _mix64(((genv & 0xFFFFFFFF) * 0x100000001B3 + 0x1234567) & _M64))
    h = _mix64(h ^ ((((episode & 0xFFFFFFFF) << 32) | (k & 0xFFFFFFFF)) & _M64))
    return float(h >> 11) * (1.0 / 9007199254740992.0)


def device_rsi_frame(seed, genv, episode, n_frames):
    """The mocap frame reset_env draws for (seed, global env id, episode counter)."""
    return min(int(device_rng_uniform(seed, genv, episode, 0) * float(n_frames)), n_frames - 1)
