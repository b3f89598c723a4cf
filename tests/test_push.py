"""External pushes without a GPU (include/dmenv.h "EXTERNAL PUSHES"; csrc/push_kernel.h): the numpy restatement against central differences of the CPU
oracle, the push kernels' waves on the wave testbench against the restatement, the schedule's launch against the host mirror, the mirror's own properties,
and the header against its Python mirror."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.perturb import PushSchedule, ScheduleMirror
from tests import helpers as H
from tests import push_cases as PC
from tests import push_numpy as PN

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "dmenv.h")
N = 13


def emu_batch(n, flags=0):
    from tests.emu_push.emu_push import EmuPushBatch
    mc = H.mocap()
    return EmuPushBatch(H.compiled_model(), mc.data_config, mc.data_vel, n, flags=flags, mocap_dt=mc.dt)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------------
def test_jacobian_matches_central_differences_of_the_oracle():
    """J_b of push_numpy (oracle kinematics + the compiled model's axes) against central differences of the oracle's xipos, step 1e-6: every body at three
    varied states, 1e-7 absolute — the difference formula's own error is eps^2 |x'''| / 6 ~ 1e-12 of truncation and 1e-16 |x| / eps ~ 1e-10 of rounding."""
    from oracle import oracle as O
    cm = H.compiled_model()
    od = O.Data(H.oracle_model())
    _idx, q, _v, _ws = PC.states(8)
    worst = 0.0
    for e in (1, 2, 3):                  # a perturbed pose, one with limits violated, one with a random orientation
        for b in range(1, 14):
            xpos, xmat, xipos, _M = PN.oracle_kinematics(od, q[e])
            J = PN.jacobian(cm, q[e], xpos.copy(), xmat.copy(), xipos.copy(), b)
            worst = max(worst, float(np.abs(J - PN.jacobian_fd(od, q[e], b)).max()))
    print("J_b against central differences: max abs %.3e" % worst)
    assert worst <= 1e-7


# ---- the kernels' waves on the testbench ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pushed():
    """one batch of 13 varied states, env e pushed on body e + 1: (batch, qvel before, the fields a push must not touch, before)"""
    b = emu_batch(N)
    idx, q, v, ws = PC.states(N)
    PC.load(b, idx, q, v, ws)
    v0 = b.get(A.F_QVEL).copy()
    keep = PC.untouched_fields(b)
    b.push(np.arange(N) % 13 + 1, PC.impulses(N))
    return b, v0, keep


def test_push_wave_matches_the_restatement_on_every_body(pushed):
    b, v0, keep = pushed
    ref = PC.reference_dqvel(N)
    dv = b.get(A.F_QVEL) - v0
    errs = [H.rel_err(dv[e], ref[e]) for e in range(N)]
    print("k_push_now on the testbench against push_numpy: max rel err %.3e" % max(errs))
    assert max(errs) <= 1e-9
    assert min(float(np.abs(ref[e]).max()) for e in range(N)) > 1e-3          # (every env was really pushed)
    PC.assert_untouched(b, keep)


def test_zero_impulse_body_zero_and_mask_zero_leave_qvel_bitwise():
    b = emu_batch(4)
    idx, q, v, ws = PC.states(4)
    v = v.copy(); v[0, 7] = -0.0                       # a negative zero survives too
    PC.load(b, idx, q, v, ws)
    v0 = b.get(A.F_QVEL).copy(); keep = PC.untouched_fields(b)
    P = PC.impulses(4)
    b.push([3, 0, 5, 14], np.vstack([np.zeros(3), P[1], P[2], P[3]]), mask=[1, 1, 0, 1])      # zero impulse | body 0 | masked out | no such body
    assert v0.tobytes() == b.get(A.F_QVEL).tobytes()
    PC.assert_untouched(b, keep)
    b.push([3, 0, 5, 2], P, mask=[1, 1, 0, 0])
    v1 = b.get(A.F_QVEL)
    assert v0[1:].tobytes() == v1[1:].tobytes() and np.abs(v1[0] - v0[0]).max() > 1e-3
    PC.assert_untouched(b, keep)


def test_two_pushes_equal_the_push_of_their_sum():
    n = 6
    idx, q, v, ws = PC.states(n)
    P1, P2 = PC.impulses(n, seed=21), PC.impulses(n, seed=22)
    body = np.array([1, 4, 7, 10, 13, 5])
    a, b = emu_batch(n), emu_batch(n)
    PC.load(a, idx, q, v, ws); PC.load(b, idx, q, v, ws)
    a.push(body, P1); a.push(body, P2)
    b.push(body, P1 + P2)
    assert H.rel_err(a.get(A.F_QVEL) - v, b.get(A.F_QVEL) - v) <= 1e-9


# ---- the schedule against the mirror ---------------------------------------------------------------------------------------------------------------------------
def sched_batch(n, env_offset=0, first=0):
    b = emu_batch(n, flags=1 | 2)                    # contact-free, limit-free steps: the schedule reads the episode counter alone
    b.set_option(A.OPT_SEED, PC.SEED); b.set_option(A.OPT_ENV_OFFSET, env_offset)
    idx, q, v, ws = PC.states(5)
    PC.load(b, idx[first:first + n], q[first:first + n], v[first:first + n], ws[first:first + n])
    b.set_push_schedule(PC.busy_schedule())
    return b


@pytest.fixture(scope="module")
def schedule_run():
    """40 steps of 5 envs with dm_batch_reset on a mask before step 17, held to the mirror at every step (the run asserts); the trace is shared"""
    b = sched_batch(5)
    mask = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    trace, begun, seen = PC.run_schedule_against_mirror(b, 5, 40, PC.busy_schedule(), reset_at=17, reset_mask=mask)
    return b, trace, begun, seen


def test_schedule_launch_follows_the_mirror_every_step(schedule_run):
    b, trace, begun, seen = schedule_run
    ep = b.get(A.F_EPISODE)
    assert list(ep) == [0, 1, 0, 1, 1]                # the counters diverged, and the run above held through it
    assert begun.min() >= 3 and min(len(s) for s in seen) >= 2


def test_schedule_is_the_same_under_env_offset_sharding(schedule_run):
    _b, trace, _begun, _seen = schedule_run
    lo, hi = sched_batch(3, 0, 0), sched_batch(2, 3, 3)
    mask = np.array([0, 1, 0, 1, 1], dtype=np.uint8)
    rng = np.random.RandomState(3)
    for t in range(20):
        if t == 17:
            lo.reset(0, 1, mask[:3]); hi.reset(0, 1, mask[3:])
        a = rng.randn(5, A.NU) * 0.3
        lo.step(a[:3]); hi.step(a[3:])
        st = np.vstack([lo.get(A.F_PUSH_STATE), hi.get(A.F_PUSH_STATE)]); F = np.vstack([lo.get(A.F_PUSH_FORCE), hi.get(A.F_PUSH_FORCE)])
        assert np.array_equal(st, trace[t][0]) and F.tobytes() == trace[t][1].tobytes(), t


def test_schedule_push_equals_the_scripted_push_of_its_recorded_force():
    """the twin on the testbench: a scheduled batch against a batch without a schedule that is given push(body, F h) from the first one's records before
    each step — one device function applies both, so state and outputs agree bit for bit"""
    n, cm = 3, H.compiled_model()
    a = sched_batch(n)
    b = sched_batch(n); b.set_push_schedule(None)
    mirror = ScheduleMirror(PC.busy_schedule(), n, seed=PC.SEED)
    rng = np.random.RandomState(9)
    pushes = 0
    for t in range(8):
        body, _F = mirror.step(a.get(A.F_EPISODE))
        act = rng.randn(n, A.NU) * 0.3
        oa = a.step(act)
        F = a.get(A.F_PUSH_FORCE)
        b.push(body, F * (cm.timestep * 1.0))
        ob = b.step(act)
        pushes += int((body > 0).sum())
        for x, y in zip(oa, ob):
            assert x.tobytes() == y.tobytes(), t
        for f in (A.F_QPOS, A.F_QVEL, A.F_QACC_WARMSTART):
            assert a.get(f).tobytes() == b.get(f).tobytes(), (t, f)
    assert pushes >= 6


# ---- the mirror's own properties ---------------------------------------------------------------------------------------------------------------------------------
def test_mirror_draws_lie_inside_their_bounds_and_only_masked_bodies_are_drawn():
    s = PushSchedule(bodies=["root", "chest", 9], force=(80.0, 120.0), duration=(2, 4), wait=(1, 5), z=(-0.25, 0.5))
    allowed = set(s.body_list())
    assert allowed == {1, 2, 9}
    m = ScheduleMirror(s, 6, seed=77, env_offset=100)
    ep = np.zeros(6, dtype=np.int32)
    bodies, begun = set(), 0
    for t in range(200):
        if t == 90:
            ep[::2] += 1
        before = m.state.copy()
        body, F = m.step(ep)
        for e in range(6):
            st = m.state[e]
            if body[e]:
                bodies.add(int(body[e]))
                mag = float(np.linalg.norm(F[e]))
                assert 80.0 - 1e-9 <= mag <= 120.0 + 1e-9 and -0.25 - 1e-12 <= F[e, 2] / mag <= 0.5 + 1e-12
                if st[4] != before[e, 4] or (st[0] != before[e, 0] and st[4] > 0):       # a push began this step: one of its steps is done
                    begun += 1
                    assert 2 <= st[2] + 1 <= 4
                if st[2] == 0:                                                            # ... and ended: the wait that follows it
                    assert 1 <= st[1] <= 5
            assert 0 <= st[1] <= 5 and 0 <= st[2] <= 3
    assert bodies == allowed and begun >= 6 * 20


def test_busy_schedule_begins_three_pushes_on_two_bodies_within_24_steps():
    """asserted on the mirror alone, so that the device tests that hold the device to the mirror are not vacuous"""
    for n, off in ((5, 0), (8, 0), (13, 0)):
        m = ScheduleMirror(PC.busy_schedule(), n, seed=PC.SEED, env_offset=off)
        ep = np.zeros(n, dtype=np.int32)
        seen = [set() for _ in range(n)]
        for t in range(24):
            c0 = m.state[:, 4].copy()
            body, _F = m.step(ep)
            for e in range(n):
                if m.state[e, 4] > c0[e]:
                    seen[e].add(int(body[e]))
        assert m.state[:, 4].min() >= 3 and min(len(s) for s in seen) >= 2, (n, m.state[:, 4], seen)


def test_push_schedule_validates_and_parses():
    s = PushSchedule.parse("bodies=deepmimic,force=50:200,duration=2:6,wait=30:90,z=-0.2:0.2")
    assert s.bodies == PushSchedule("deepmimic", (50, 200)).bodies and s.force == (50.0, 200.0) and s.duration == (2, 6) and s.wait == (30, 90) and s.z == (-0.2, 0.2)
    assert PushSchedule.parse("bodies=root+3,force=100").body_list() == [1, 3] and PushSchedule.parse("none") is None
    assert PushSchedule.coerce(dict(bodies=[2], force=5.0)).force == (5.0, 5.0)
    for bad in (dict(bodies=[], force=1.0), dict(bodies=[1], force=(2.0, 1.0)), dict(bodies=[1], force=(-1.0, 1.0)), dict(bodies=[1], force=float("inf")),
                dict(bodies=[1], force=1.0, duration=(0, 2)), dict(bodies=[1], force=1.0, wait=(-1, 2)), dict(bodies=[1], force=1.0, z=(-1.5, 0.0)),
                dict(bodies=[14], force=1.0), dict(bodies=["elbow"], force=1.0)):
        with pytest.raises(ValueError):
            PushSchedule(**bad)
    with pytest.raises(ValueError):
        PushSchedule.parse("bodies=root,strength=3")


# ---- the header ------------------------------------------------------------------------------------------------------------------------------------------------
def test_header_and_python_mirror_agree():
    text = open(HEADER).read()
    assert int(re.search(r"#define DM_ABI_VERSION (\d+)", text).group(1)) == A.ABI_VERSION == 9
    assert int(re.search(r"DM_F_PUSH_STATE = (\d+)", text).group(1)) == A.F_PUSH_STATE == 20
    assert int(re.search(r"DM_F_PUSH_FORCE = (\d+)", text).group(1)) == A.F_PUSH_FORCE == 21
    assert A.FIELD_SPEC[A.F_PUSH_STATE] == (np.int32, (5,)) and A.FIELD_SPEC[A.F_PUSH_FORCE] == (np.float64, (3,))
    body = re.search(r"typedef struct \{([^}]*)\} dm_push_desc;", text).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in A.PushDesc._fields_]
    assert C.sizeof(A.PushDesc) == 4 + 4 * 4 + 4 + 4 * 8          # uint32, four int32, padding to 8, four doubles
    assert "dm_batch_push" in A.EXPORTS and "dm_batch_set_push_schedule" in A.EXPORTS


@pytest.mark.parametrize("dtype", [64, 32])
def test_argument_errors_are_refused_in_both_libraries(dtype):
    L = A.load(dtype)
    body = np.zeros(1, dtype=np.int32); imp = np.zeros((1, 3))
    assert L.dm_batch_push(None, body.ctypes.data, imp.ctypes.data, None, A.PTR_HOST) == -1 and b"dm_batch_push" in L.dm_last_error()
    ok = PushSchedule([1, 2], (10.0, 20.0), duration=(1, 2), wait=(0, 3)).desc()
    assert L.dm_batch_set_push_schedule(None, C.byref(ok)) == -1 and b"null batch" in L.dm_last_error()
    for field, val, word in (("bodies", 1, b"bodies"), ("bodies", 1 << 14, b"bodies"), ("wait_min", -1, b"wait"), ("wait_max", -1, b"wait"),
                             ("duration_min", 0, b"duration"), ("duration_max", 0, b"duration"), ("force_min", -1.0, b"force"), ("force_max", float("inf"), b"force"),
                             ("force_min", float("nan"), b"force"), ("z_min", -1.5, b"z_min"), ("z_max", 1.5, b"z_min"), ("z_min", float("nan"), b"z_min")):
        d = PushSchedule([1, 2], (10.0, 20.0), duration=(1, 2), wait=(0, 3)).desc()
        setattr(d, field, val)
        assert L.dm_batch_set_push_schedule(None, C.byref(d)) == -1 and word in L.dm_last_error(), field
