"""The packed step at each capacity of its row builder (csrc/slot_kernel.h slot_rows: 16 limit rows, 8 contact pairs, 13 contacts, 32 broad-phase candidates,
16 candidates per narrow-phase trip), on the wave testbench: the states of tests/golden/slot_capacities.npz sit AT a capacity or ONE PAST it
(tools/make_capacity_golden.py found them with the oracle and tests/rows_numpy.py alone) and share their waves as tests/capacity_cases.py says.

  * the fixture still sits on its edges: every recorded count is recomputed from rows_numpy and the oracle, and each entry's own condition is asserted again;
  * one step of the lean and the three-set per-step launches and of a one-step horizon launch counts every "past" environment under its reason exactly once and
    nothing else (dm_batch_redo_total's counters: EmuBatch.redo_reasons);
  * four steps agree with the oracle env by env to 1e-9, with equal done flags, row counts, contact counts and contact geom lists; the horizon launch and the
    three-set per-step launches agree bit for bit, and so do the lean launches up to the step at which an environment first passes 32 rows;
  * behind every step of the horizon launch the slots hold, for EVERY environment of the wave, the observation row just written — what the fused policy reads
    (slot_step.h slot_rollout reloads it after an in-wave re-step has overwritten the slots' LDS);
  * the narrow-phase fixtures (capsule-box and box-box poses, which the one-env kernel's forward evaluation is held to elsewhere) take one step from rest on
    the packed path — the packed emission of the box staging slots — and agree with the oracle.  No pose sits on a discontinuity of the step map: none is left out."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from tests import capacity_cases as CC
from tests import helpers as H
from tests import rows_numpy as RW

ALLOWED_UNREACHED = {"contacts_at", "contacts_past", "candidates_past"}
_RUNS = {}


def test_the_fixture_holds_every_edge_but_the_three_that_may_be_missing():
    ent, unreached = CC.fixture()
    assert set(unreached) <= ALLOWED_UNREACHED, unreached
    for edge in ("limits_at", "limits_past", "frames_at", "frames_past", "candidates_16", "candidates_17", "candidates_20plus", "candidates_at", "norow"):
        assert edge in ent, edge
    for edge in ALLOWED_UNREACHED:
        assert (edge in ent) != (edge in unreached), edge


def test_every_recorded_count_is_what_numpy_and_the_oracle_give_and_the_states_sit_on_their_edges():
    from oracle import oracle as O
    ent, _u = CC.fixture()
    cm = H.compiled_model()
    od = O.Data(H.oracle_model())
    caps = RW.CAPS
    for name, e in ent.items():
        c = RW.counts_at(cm, od, e["qpos"], e["qvel"], e["qacc_warmstart"])
        assert {k: c[k] for k in e["counts"]} == e["counts"], (name, c, e["counts"])
        assert c["late_contacts"] == e["late_contacts"], name
        _o, _d, pk = RW.step_maxima(od, e["action"])
        assert pk == e["peaks"], (name, pk, e["peaks"])
        assert c["rows"] <= caps["rows"], name
        kind = name.rsplit("_", 1)[-1]
        own = name.split("_")[0]
        calm = c["candidates"] <= 14 or 19 <= c["candidates"] <= 30              # two away from the trip edge and inside the candidate capacity
        if kind == "past":
            assert c[own] == caps[own] + 1, (name, c)
            assert all(c[k] <= caps[k] for k in caps if k != own), (name, c)          # only its own capacity is exceeded at the first evaluation
            assert own == "candidates" or calm, (name, c)
        else:
            assert all(c[k] <= caps[k] for k in caps) and all(pk[k] <= caps[k] for k in pk), (name, c, pk)      # inside every capacity over the whole step
            if kind == "at":
                assert c[own] == caps[own] and (own not in pk or pk[own] == caps[own]), (name, c, pk)
            if own != "candidates":
                assert calm, (name, c)
    assert ent["candidates_16"]["counts"]["candidates"] == RW.TRIP and ent["candidates_17"]["counts"]["candidates"] == RW.TRIP + 1
    assert 20 <= ent["candidates_20plus"]["counts"]["candidates"] <= 30
    for name in ("candidates_17", "candidates_20plus", "candidates_at"):      # a contact among the candidates 16 and up: the second trip finds a row
        assert ent[name]["late_contacts"] >= 1, name
    assert ent["norow"]["counts"]["rows"] == 0
    for k in range(6):
        assert 1 <= ent["light_%d" % k]["counts"]["rows"] <= 11 and ent["light_%d" % k]["counts"]["candidates"] < 8


def test_the_waves_cover_the_five_kinds():
    ent, _u = CC.fixture()
    waves = [(case, i, w) for case in CC.CASES for i, w in enumerate(CC.CASES[case])]
    past = lambda w: [n for n in w if n in CC.PAST_REASON]
    assert sum(len(w) for _c, _i, w in waves) <= 40
    assert any(len(w) == 4 and len(past(w)) == 1 for _c, _i, w in waves), "one environment leaves while three stay"
    assert any(len({CC.PAST_REASON[n] for n in past(w)}) >= 2 and len(past(w)) < len(w) for _c, _i, w in waves), "two leave for different reasons"
    assert any(len(w) == 4 and len(past(w)) == 4 for _c, _i, w in waves), "all four slots past a capacity"
    assert all(len(CC.CASES[case][-1]) < 4 for case in ("several_leave", "none_leaves")), "a last wave that is partly filled"
    case, i = CC.SLOT3_WAVE
    w = CC.CASES[case][i]
    cand = [ent[n]["counts"]["candidates"] for n in w]
    assert cand[3] >= 17 and all(c < 8 for c in cand[:3]), cand
    for _c, _i, w in waves:                                                    # an edge state next to a state without rows
        assert "norow" in w or len(w) < 4 or len(past(w)) == 4, w
    assert not past([n for w in CC.CASES["none_leaves"] for n in w])


def _batch(case, mode):
    from tests.emu.emu import EmuBatch
    mc = H.mocap()
    names, f, q, v, ws, acts = CC.states(case)
    b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, len(q), 0)
    b.set_option(A.OPT_PACKED, mode)
    H.start(b, f, q, v, ws=ws)
    return b, names, acts


def _run(case, form):
    """form: "lean" / "three_set" (per-step launches, DM_OPT_PACKED 1 / 2) or "horizon" -> the rows, the state fields after every step the form shows them at,
    and the reason counters after the first step (the horizon launch's: after a one-step launch of a batch of its own)"""
    if (case, form) in _RUNS:
        return _RUNS[(case, form)]
    mode = 2 if form == "three_set" else 1
    b, names, acts = _batch(case, mode)
    n = len(names)
    out = {}
    if form == "horizon":
        one, _names, _a = _batch(case, mode)
        one.rollout(acts[:1])
        out["reasons"] = one.redo_reasons()
        obs, rew, done, pin = b.rollout(acts, policy_inputs=True)
        out["policy_inputs"] = pin
    else:
        obs = np.zeros((CC.T, n, 56)); rew = np.zeros((CC.T, n)); done = np.zeros((CC.T, n), dtype=np.uint8)
        per = dict(nefc=[], ncon=[], geoms=[], qacc=[], solver_iter=[], redo=[])
        for t in range(CC.T):
            b.step(acts[t], 1, out=(obs[t], rew[t], done[t]))
            if t == 0:
                out["reasons"] = b.redo_reasons()
            per["nefc"].append(b.get(A.F_NEFC)); per["ncon"].append(b.get(A.F_NCON)); per["geoms"].append(b.get(A.F_CONTACT_GEOMS))
            per["qacc"].append(b.get(A.F_QACC_WARMSTART)); per["solver_iter"].append(b.get(A.F_SOLVER_ITER)); per["redo"].append(b.redo_total())
        out.update({k + "_steps": np.array(x) for k, x in per.items()})
    out.update(obs=obs, rew=rew, done=done, qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL), qacc=b.get(A.F_QACC_WARMSTART), solver_iter=b.get(A.F_SOLVER_ITER),
               nefc=b.get(A.F_NEFC))
    _RUNS[(case, form)] = out
    return out


@pytest.mark.parametrize("form", ["lean", "three_set", "horizon"])
@pytest.mark.parametrize("case", list(CC.CASES))
def test_one_step_counts_every_environment_past_a_capacity_under_its_reason_and_nothing_else(case, form):
    got = _run(case, form)["reasons"]
    want = CC.expected_reasons(CC.names_of(case))
    print(case, form, dict(zip(RW.REASON_NAMES, got)))
    assert got == want, "%s on %s: counted %s, expected %s" % (case, form, dict(zip(RW.REASON_NAMES, got)), dict(zip(RW.REASON_NAMES, want)))
    assert got[2] == 0 and got[5] == 0


@pytest.mark.parametrize("form", ["lean", "three_set", "horizon"])
@pytest.mark.parametrize("case", list(CC.CASES))
def test_four_steps_agree_with_the_oracle_env_by_env(case, form):
    r, want = _run(case, form), CC.oracle(case)
    err = CC.rel_err(r["obs"], want["obs"])
    print(case, form, "worst rel err vs oracle %.3e" % err.max())
    assert err.max() < 1e-9, (np.argwhere(err >= 1e-9).tolist(), err.max())
    assert np.array_equal(r["done"], want["done"])
    if form != "horizon":
        assert np.array_equal(r["nefc_steps"], want["nefc"]) and np.array_equal(r["ncon_steps"], want["ncon"])
        assert np.array_equal(r["geoms_steps"].reshape(want["geoms"].shape), want["geoms"])
    else:
        assert np.array_equal(r["nefc"], want["nefc"][-1])


@pytest.mark.parametrize("case", list(CC.CASES))
def test_the_forms_that_share_step_code_agree_bit_for_bit(case):
    ref, hor, lean = _run(case, "three_set"), _run(case, "horizon"), _run(case, "lean")
    for k in ("obs", "rew", "done", "qpos", "qvel", "qacc", "solver_iter", "nefc"):
        assert np.array_equal(hor[k], ref[k]), "%s differs between the horizon and the three-set per-step launches" % k
    # the lean launches hand an environment that passes 32 rows inside a step to the one-env code (its arithmetic): compared up to that step, and not at all
    # from the step at which the lean launches re-step more than the three-set launches' own re-steps and the row counts at the steps' ends explain
    over = ref["nefc_steps"] > A.PACKED_MAXROWS_PER_STEP
    first = np.where(over.any(0), over.argmax(0), CC.T)
    explained = ref["redo_steps"] + np.cumsum(over.sum(1))
    unexplained = lean["redo_steps"] > explained
    clean = int(unexplained.argmax()) if unexplained.any() else CC.T
    assert clean >= 1, "nothing left to compare: choose other states"
    for e in range(ref["obs"].shape[1]):
        for t in range(min(int(first[e]), clean)):
            assert np.array_equal(lean["obs"][t, e], ref["obs"][t, e]), (e, t)
            assert np.array_equal(lean["qacc_steps"][t, e], ref["qacc_steps"][t, e]) and lean["solver_iter_steps"][t, e] == ref["solver_iter_steps"][t, e], (e, t)


@pytest.mark.parametrize("case", list(CC.CASES))
def test_behind_every_horizon_step_the_slots_hold_each_environments_own_observation(case):
    r = _run(case, "horizon")
    assert np.isfinite(r["policy_inputs"]).all(), "a slot's policy inputs were never read"
    bad = np.argwhere((r["policy_inputs"] != r["obs"]).any(-1))
    assert bad.size == 0, "(step, env) whose slot does not hold the observation row the step wrote: %s of %s" % (bad.tolist(), CC.names_of(case))


@pytest.mark.parametrize("form", ["lean", "three_set", "horizon"])
def test_the_narrow_phase_fixtures_take_a_packed_step_that_agrees_with_the_oracle(form):
    from tests.emu.emu import EmuBatch
    mc = H.mocap()
    files, qs = CC.narrow_poses()
    want = CC.narrow_oracle()
    n = len(qs)
    b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, n, 0)
    b.set_option(A.OPT_PACKED, 2 if form == "three_set" else 1)
    H.start(b, np.zeros(n, dtype=np.int32), qs, np.zeros((n, 34)))
    act = np.zeros((1, n, 28))
    if form == "horizon":
        obs, _rew, done = b.rollout(act)
    else:
        o, _r, d = b.step(act[0], 1)
        obs, done = o[None], d[None]
    err = CC.rel_err(obs[0], want["obs"])
    print(form, "worst rel err vs oracle %.3e" % err.max(), "re-stepped", b.redo_reasons(), "inside every capacity: %d of %d" % (want["inside"].sum(), n))
    assert err.max() < 1e-9, [(files[e], e, err[e]) for e in np.nonzero(err >= 1e-9)[0]]
    assert np.array_equal(done[0], want["done"])
    assert np.array_equal(b.get(A.F_NEFC), want["nefc"]) and np.array_equal(b.get(A.F_NCON), want["ncon"])
    assert np.array_equal(b.get(A.F_CONTACT_GEOMS).reshape(want["geoms"].shape), want["geoms"])
    assert b.redo_total() <= n - int(want["inside"].sum()), "a pose inside every capacity was handed to the one-env code: %s" % (b.redo_reasons(),)
    assert int(want["inside"].sum()) >= n // 2, "most poses must stay on the packed path, or this test does not see its emission"
