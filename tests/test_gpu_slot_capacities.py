"""The packed step at each capacity of its row builder (csrc/slot_kernel.h slot_rows: 16 limit rows, 8 contact pairs, 13 contacts, 32 broad-phase candidates,
16 candidates per narrow-phase trip), on the device: the waves of tests/capacity_cases.py — states AT a capacity and ONE PAST it (tests/golden/
slot_capacities.npz) beside a no-row state, a light state and an edge state of another capacity, 36 environments — through the per-step packed launches
(`packed`, `packed-ext`), the step queue as deep as the run, the horizon launch (`rollout`) and the horizon launch with the fused policy (`rollout-act`), the
last three with DM_OPT_PACKED 1 and 2.  tests/test_slot_capacities.py holds the same cases on the wave testbench.

  a. after ONE step of every form dm_batch_redo_total has counted every environment past a capacity under its reason, exactly once, and nothing else;
  b. four steps agree with the oracle env by env to 1e-9 with equal done flags; after every step of the per-step forms DM_F_NEFC, DM_F_NCON and
     DM_F_CONTACT_GEOMS are the oracle's; the queue and the horizon launch give the three-set per-step launches' bits, the lean per-step launches too for as
     long as an environment stays within 32 rows (tests/test_gpu_slot_variant_boundaries.py's rule);
  c. on `rollout-act` the action row t + 1 and the value t of EVERY environment — the re-stepped ones and their wave partners, whose slots the in-wave re-step
     overwrote — are dm_policy_act's on the observation row t (test_fused_policy_step_equals_step_then_act's bars: 1e-5 on actions, 1e-4 relative on values),
     and the steps that follow a re-step, which run without the kinematics carry, agree with the oracle under those actions like every other;
  d. the narrow-phase fixtures (capsule-box, box-box poses) take one step from rest through `packed`, `packed-ext` and `rollout` and agree with the oracle,
     contact counts and geom lists included: the packed emission of the box staging slots on the poses the one-env kernel is held to elsewhere."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import DPVecEnv
from tests import capacity_cases as CC
from tests import gpu_batch as GB
from tests import helpers as H
from tests import rows_numpy as RW

pytestmark = pytest.mark.gpu
T = CC.T
# (form of tests/gpu_batch.py, DM_OPT_PACKED): `packed` is the option's 1 and `packed-ext` its 2; the other forms take both
RUNS = [("packed", 1), ("packed-ext", 2), ("queue", 1), ("queue", 2), ("rollout", 1), ("rollout", 2), ("rollout-act", 1), ("rollout-act", 2)]
OPEN_LOOP = [r for r in RUNS if r[0] != "rollout-act"]
_CACHE = {}


def _form(name, steps):
    return GB.FORMS[name]._replace(queue_depth=steps) if name == "queue" else GB.FORMS[name]


def _make(n, mode):
    env = DPVecEnv(n, motion="walk", device=0, reward="alive", autoreset=None, packed=True, frame_skip=1, diagnostics=True)      # (the contact geom lists are read)
    env.batch.set_option(A.OPT_PACKED, mode)
    return env


def _run(case, name, mode, steps):
    """`steps` steps of the case's environments through the form -> rows and final state; the per-step forms' state after every step as well"""
    key = (case, name, mode, steps)
    if key in _CACHE:
        return _CACHE[key]
    _names, f, q, v, ws, acts = CC.states(case)
    n = len(q)
    env = _make(n, mode)
    b = env.batch
    GB.start(b, f, q, v, ws=ws)
    form = _form(name, steps)
    pol = W = None
    if form.policy:
        pol, W = GB.fused_policy()
        ac, ob, rew, dn, vp = GB.horizon_rows(steps, n, a0=acts[0])
    else:
        ac, ob, rew, dn, vp = GB.horizon_rows(steps, n, act=acts[:steps])
    per = dict(nefc=[], ncon=[], geoms=[], redo=[])
    redo0 = b.redo_reasons()

    def read(t):
        per["nefc"].append(b.get(A.F_NEFC)); per["ncon"].append(b.get(A.F_NCON)); per["geoms"].append(b.get(A.F_CONTACT_GEOMS)); per["redo"].append(b.redo_total() - redo0[0])
    GB.issue_steps(b, form, ac, ob, rew, dn, 1, pol=pol, W=W, vp=vp, between=read if name in ("packed", "packed-ext") else None)
    out = dict(obs=ob.cpu().numpy(), rew=rew.cpu().numpy(), done=dn.cpu().numpy(), ac=ac.cpu().numpy(), vp=vp.cpu().numpy(), qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL),
               qacc=b.get(A.F_QACC_WARMSTART), solver_iter=b.get(A.F_SOLVER_ITER), nefc=b.get(A.F_NEFC),
               reasons=[int(x - y) for x, y in zip(b.redo_reasons(), redo0)])
    out.update({k + "_steps": np.array(x) for k, x in per.items() if x})
    if form.policy:                                   # dm_policy_act on the rows the launch wrote, with the launch's seed and counters
        ref_ac = torch.zeros_like(ac); ref_vp = torch.zeros_like(vp)
        for t in range(steps):
            pol._counter = 7 + t - 1
            pol.act(True, ob[t], out=ref_ac[t + 1], vpred_out=ref_vp[t])
        torch.cuda.synchronize()
        out.update(ref_ac=ref_ac.cpu().numpy(), ref_vp=ref_vp.cpu().numpy())
    env.close()
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("case", list(CC.CASES))
def test_one_step_counts_every_environment_past_a_capacity_under_its_reason_and_nothing_else(case):
    want = CC.expected_reasons(CC.names_of(case))
    for name, mode in RUNS:
        got = _run(case, name, mode, 1)["reasons"]
        print(case, name, mode, dict(zip(RW.REASON_NAMES, got)))
        assert got == want, "%s on %s (DM_OPT_PACKED %d): counted %s, expected %s" % (case, name, mode, dict(zip(RW.REASON_NAMES, got)), dict(zip(RW.REASON_NAMES, want)))
        assert got[2] == 0 and got[5] == 0


@pytest.mark.parametrize("case", list(CC.CASES))
def test_four_steps_agree_with_the_oracle_and_the_forms_with_one_another(case):
    want = CC.oracle(case)
    runs = {(name, mode): _run(case, name, mode, T) for name, mode in OPEN_LOOP}
    for key, r in runs.items():
        err = CC.rel_err(r["obs"], want["obs"])
        print(case, key, "worst rel err vs oracle %.3e" % err.max(), "re-stepped", r["reasons"])
        assert err.max() < 1e-9, (key, np.argwhere(err >= 1e-9).tolist(), err.max())
        assert np.array_equal(r["done"], want["done"]), key
        assert np.array_equal(r["nefc"], want["nefc"][-1]), key
        if "nefc_steps" in r:
            assert np.array_equal(r["nefc_steps"], want["nefc"]) and np.array_equal(r["ncon_steps"], want["ncon"]), key
            assert np.array_equal(r["geoms_steps"].reshape(want["geoms"].shape), want["geoms"]), key
    ref = runs[("packed-ext", 2)]
    for key in (("queue", 2), ("rollout", 2), ("queue", 1), ("rollout", 1)):
        for k in ("obs", "rew", "done", "qpos", "qvel", "qacc", "solver_iter", "nefc"):
            assert np.array_equal(runs[key][k], ref[k]), "%s differs between %s and the three-set per-step launches" % (k, key)
    # the lean per-step launches: the same bits for as long as an environment stays within 32 rows, and nothing from the step on at which they re-step more than
    # the three-set launches' own re-steps and the row counts at the steps' ends explain (an environment that passed 32 rows inside a step)
    lean = runs[("packed", 1)]
    over = ref["nefc_steps"] > A.PACKED_MAXROWS_PER_STEP
    first = np.where(over.any(0), over.argmax(0), T)
    explained = ref["redo_steps"] + np.cumsum(over.sum(1))
    unexplained = lean["redo_steps"] > explained
    clean = int(unexplained.argmax()) if unexplained.any() else T
    print(case, "lean re-steps", lean["redo_steps"].tolist(), "three-set", ref["redo_steps"].tolist(), "first step above 32 rows", first.tolist(), "compared steps", clean)
    assert clean >= 1, "nothing left to compare: choose other states"
    for e in range(ref["obs"].shape[1]):
        upto = min(int(first[e]), clean)
        for t in range(upto):
            assert np.array_equal(lean["obs"][t, e], ref["obs"][t, e]), "env %d differs between the lean and the three-set per-step launches at step %d" % (e, t)
        if upto == T:
            for k in ("qpos", "qvel", "qacc", "solver_iter", "nefc"):
                assert np.array_equal(lean[k][e], ref[k][e]), (k, e)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("case", list(CC.CASES))
def test_the_fused_policy_acts_on_every_environments_own_observation_after_an_in_wave_restep(case, mode):
    from oracle import oracle as O
    names, _f, q, v, ws, _acts = CC.states(case)
    r = _run(case, "rollout-act", mode, T)
    n = len(names)
    # c. the policy's rows: every environment, every step
    a_err = np.abs(r["ac"][1:] - r["ref_ac"][1:]).max(axis=-1)                               # [T, n]
    v_err = np.abs(r["vp"] - r["ref_vp"]) / max(1.0, float(np.abs(r["ref_vp"]).max()))
    print(case, mode, "worst action difference %.2e, value %.2e; re-stepped %s" % (a_err.max(), v_err.max(), r["reasons"]))
    assert a_err.max() < 1e-5, "(step, env) whose action is not the policy's on its own observation: %s of %s" % (np.argwhere(a_err >= 1e-5).tolist(), names)
    assert v_err.max() < 1e-4, np.argwhere(v_err >= 1e-4).tolist()
    if any(x in CC.PAST_REASON for x in names):
        assert r["reasons"][0] >= 1                                                           # the launch re-stepped inside its waves
    # the steps under the policy's actions, the one after a re-step among them, against the oracle
    om = H.oracle_model()
    obs = np.zeros((T, n, 56)); done = np.zeros((T, n), dtype=np.uint8)
    for e in range(n):
        od = O.Data(om); od.reset(); od.set("qacc_warmstart", ws[e]); od.set_state(q[e], v[e])
        for t in range(T):
            o, _r, d, _ = od.env_step(r["ac"][t, e])
            obs[t, e] = o; done[t, e] = d
    err = CC.rel_err(r["obs"], obs)
    print(case, mode, "worst rel err vs oracle %.3e" % err.max())
    assert err.max() < 1e-9, (np.argwhere(err >= 1e-9).tolist(), err.max())
    assert np.array_equal(r["done"], done)


@pytest.mark.parametrize("name,mode", [("packed", 1), ("packed-ext", 2), ("rollout", 1)])
def test_the_narrow_phase_fixtures_take_a_packed_step_that_agrees_with_the_oracle(name, mode):
    files, qs = CC.narrow_poses()
    want = CC.narrow_oracle()
    n = len(qs)
    env = _make(n, mode)
    b = env.batch
    GB.start(b, np.zeros(n, dtype=np.int32), qs, np.zeros((n, 34)))
    redo0 = b.redo_total()
    ac, ob, rew, dn, _vp = GB.horizon_rows(1, n)
    GB.issue_steps(b, GB.FORMS[name], ac, ob, rew, dn, 1)
    obs, done = ob.cpu().numpy()[0], dn.cpu().numpy()[0]
    err = CC.rel_err(obs, want["obs"])
    redo = b.redo_total() - redo0
    print(name, "worst rel err vs oracle %.3e" % err.max(), "re-stepped", redo, "inside every capacity: %d of %d" % (want["inside"].sum(), n))
    assert err.max() < 1e-9, [(files[e], e, err[e]) for e in np.nonzero(err >= 1e-9)[0]]
    assert np.array_equal(done, want["done"])
    assert np.array_equal(b.get(A.F_NEFC), want["nefc"]) and np.array_equal(b.get(A.F_NCON), want["ncon"])
    assert np.array_equal(b.get(A.F_CONTACT_GEOMS).reshape(want["geoms"].shape), want["geoms"])
    assert redo <= n - int(want["inside"].sum()), "a pose inside every capacity was handed to the one-env code"
    assert int(want["inside"].sum()) >= n // 2
    env.close()
