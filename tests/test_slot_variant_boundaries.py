"""slot_kernel.h slot_forward picks its constraint-stage code from the wave's largest row count: one row set up to 16 rows, two up to 32 (whose block A10 of
A = Y Y^T is A01 transposed through LDS instead of a second build), the partial third set beyond.  These are the same sums in the same order, so a result may
not depend on the path a wave took nor on how a path forms them: the kernel source, run on the fibre testbench, must reproduce bit for bit what the commit
before the transposed block computed for waves led by 14, 15, 16, 17, 30, 31 and 32 rows with partners of 0 rows (tests/golden/
slot_variant_boundaries.npz, recorded by tools/make_slot_variant_golden.py from oracle rollouts of `walk` under N(0, 0.9^2) actions).  The testbench keeps no
constraint forces; the accelerations they produce (qacc), the states, the sweep counts and the row counts are compared."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from tests import helpers as H

BOUNDARIES = (14, 15, 16, 17, 30, 31, 32)
KEYS = ("obs", "reward", "done", "qpos", "qvel", "qacc", "solver_iter", "nefc")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(H.GOLDEN + "/slot_variant_boundaries.npz"))


def _run(g, mode, horizon):
    from tests.emu.emu import EmuBatch
    mc = H.mocap()
    n = len(g["frame"])
    acts = g["actions"]
    b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, n, 0)
    b.set_option(A.OPT_PACKED, mode)
    b.set(A.F_QACC_WARMSTART, g["qacc_warmstart0"]); b.set(A.F_TIME, np.zeros(n))
    b.set_state(g["qpos0"], g["qvel0"], frame_idx=g["frame"])
    out = {"nefc0": b.get(A.F_NEFC).copy()}
    T = acts.shape[0]
    if horizon:
        obs, rew, done = b.rollout(acts)
    else:
        obs = np.zeros((T, n, 56)); rew = np.zeros((T, n)); done = np.zeros((T, n), dtype=np.uint8)
        qacc = np.zeros((T, n, 34)); it = np.zeros((T, n), dtype=np.int32); ne = np.zeros((T, n), dtype=np.int32)
        for t in range(T):
            b.step(acts[t], 1, out=(obs[t], rew[t], done[t]))
            qacc[t] = b.get(A.F_QACC_WARMSTART); it[t] = b.get(A.F_SOLVER_ITER); ne[t] = b.get(A.F_NEFC)
        out.update(qacc_steps=qacc, solver_iter_steps=it, nefc_steps=ne)
    out.update(obs=obs, reward=rew, done=done, qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL), qacc=b.get(A.F_QACC_WARMSTART),
               solver_iter=b.get(A.F_SOLVER_ITER), nefc=b.get(A.F_NEFC), redo=np.asarray(b.redo_total()))
    return out


def test_every_boundary_class_leads_a_wave_next_to_a_partner_without_rows(golden):
    ne = golden["nefc0"]
    waves = [ne[i:i + 4] for i in range(0, len(ne), 4)]
    for b in BOUNDARIES:
        led = [w for w in waves if int(w.max()) == b]
        assert led, "no wave whose largest row count is %d" % b
        assert any((w == 0).any() for w in led), "no wave led by %d rows holds a partner without rows" % b
    assert len(waves[-1]) < 4, "the last wave is partly filled"


@pytest.mark.parametrize("form", ["per_step_three_set", "horizon", "per_step_lean"])
def test_boundary_waves_reproduce_the_recorded_bits(golden, form):
    out = _run(golden, {"per_step_three_set": 2, "horizon": 1, "per_step_lean": 1}[form], form == "horizon")
    assert np.array_equal(out["nefc0"], golden["nefc0"]), "the states' row counts moved: the fixture no longer sits on the boundaries"
    pre = "lean_" if form == "per_step_lean" else ""
    keys = KEYS + (("qacc_steps", "solver_iter_steps", "nefc_steps") if form != "horizon" else ())
    for k in keys:
        want = golden[pre + k]
        assert out[k].dtype == want.dtype and np.array_equal(out[k], want), "%s differs from the recorded values (%s)" % (k, form)
    assert int(out["redo"]) == int(golden[pre + "redo"])
