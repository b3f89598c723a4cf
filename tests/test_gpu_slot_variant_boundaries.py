"""The packed step at the row counts where slot_forward changes its constraint-stage code (slot_kernel.h: one row set up to 16 rows, two up to 32 — whose
block A10 is A01 transposed through LDS — the partial third set beyond), on the device: waves led by 14, 15, 16, 17, 30, 31 and 32 rows with partners of 0
rows (the states of tests/golden/slot_variant_boundaries.npz, placed through set_state), four steps, through the per-step packed launch, the step queue and
the horizon launch, each with the lean and the three-set per-step kernels (DM_OPT_PACKED 1 and 2).  Every form agrees with the oracle to 1e-9; the forms
agree with one another bit for bit.  The lean per-step kernel hands an environment that passes 32 rows inside a step to the one-env code (its arithmetic,
not the packed one's): such an environment is compared up to that step, and once the launch's redo counter shows a re-step that the row counts at the steps' ends do not
explain, nothing later is compared."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import DPVecEnv
from tests import helpers as H
from tests import gpu_batch as GB

pytestmark = pytest.mark.gpu
T = 4
# this file's launch-form ids -> tests/gpu_batch.py FORMS; each runs with DM_OPT_PACKED 1 and 2, the queue as deep as the run
FORMS = {"per_step": GB.FORMS["packed"], "queue": GB.FORMS["queue"]._replace(queue_depth=T), "horizon": GB.FORMS["rollout"]}
CASES = {"14_15": (0, 8), "16_17": (8, 16), "30_31": (16, 24), "32_partly_filled": (24, 30)}      # two waves of the fixture each
LEADS = {"14_15": (14, 15), "16_17": (16, 17), "30_31": (30, 31), "32_partly_filled": (32, 31)}
_ORACLE = {}


def _states(case):
    g = np.load(H.GOLDEN + "/slot_variant_boundaries.npz")
    lo, hi = CASES[case]
    n = hi - lo
    acts = np.random.RandomState(100 + lo).randn(T, n, 28) * 0.9
    return g["frame"][lo:hi], g["qpos0"][lo:hi], g["qvel0"][lo:hi], g["qacc_warmstart0"][lo:hi], g["nefc0"][lo:hi], acts


def _oracle(case):
    if case not in _ORACLE:
        from oracle import oracle as O
        _f, q, v, ws, _ne, acts = _states(case)
        om = H.oracle_model()
        n = len(q)
        obs = np.zeros((T, n, 56)); done = np.zeros((T, n), dtype=np.uint8)
        for e in range(n):
            od = O.Data(om); od.reset(); od.set("qacc_warmstart", ws[e]); od.set_state(q[e], v[e])
            for t in range(T):
                o, _r, d, _ = od.env_step(acts[t, e])
                obs[t, e] = o; done[t, e] = d
        obs.setflags(write=False); done.setflags(write=False)
        _ORACLE[case] = (obs, done)
    return _ORACLE[case]


def _run(case, form, mode):
    f, q, v, ws, ne0, acts = _states(case)
    n = len(q)
    env = DPVecEnv(n, motion="walk", device=0, reward="alive", autoreset=None, packed=True, frame_skip=1)
    b = env.batch
    b.set_option(A.OPT_PACKED, mode)
    GB.start(b, f, q, v, ws=ws)
    assert np.array_equal(b.get(A.F_NEFC), ne0), "the states' row counts moved: the fixture no longer sits on the boundaries"
    ac, ob, rew, dn, _vp = GB.horizon_rows(T, n, act=acts)
    rows = redo_steps = None
    redo0 = b.redo_total()
    if form != "horizon":
        rows = np.zeros((T, n), dtype=np.int64); redo_steps = np.zeros(T, dtype=np.int64)

    def read_rows(t):
        rows[t] = b.get(A.F_NEFC); redo_steps[t] = b.redo_total() - redo0
    GB.issue_steps(b, FORMS[form]._replace(packed=mode), ac, ob, rew, dn, 1, between=read_rows if form == "per_step" else None)
    out = dict(obs=ob.cpu().numpy(), rew=rew.cpu().numpy(), done=dn.cpu().numpy(), qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL),
               qacc=b.get(A.F_QACC_WARMSTART), solver_iter=b.get(A.F_SOLVER_ITER), nefc=b.get(A.F_NEFC), rows=rows, redo_steps=redo_steps, redo=b.redo_total() - redo0)
    env.close()
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_boundary_row_counts_on_every_packed_launch_form(case):
    _f, _q, _v, _ws, ne0, _a = _states(case)
    n = len(ne0)
    waves = [ne0[i:i + 4] for i in range(0, n, 4)]
    assert tuple(int(w.max()) for w in waves) == LEADS[case] and all((w == 0).any() for w in waves), ne0
    want_obs, want_done = _oracle(case)
    runs = {(form, mode): _run(case, form, mode) for mode in (2, 1) for form in ("per_step", "queue", "horizon")}
    for key, r in runs.items():
        err = float(np.abs(r["obs"] - want_obs).max() / max(1.0, np.abs(want_obs).max()))
        print(case, key, "rel err vs oracle %.3e" % err, "re-stepped", r["redo"])
        assert err < 1e-9, (key, err)
        assert np.array_equal(r["done"], want_done), key
    # the forms that keep up to 40 rows on the packed path: one result, bit for bit
    ref = runs[("per_step", 2)]
    for key in (("queue", 2), ("horizon", 2), ("queue", 1), ("horizon", 1)):
        for k in ("obs", "rew", "done", "qpos", "qvel", "qacc", "solver_iter", "nefc"):
            assert np.array_equal(runs[key][k], ref[k]), "%s differs between %s and the three-set per-step launches" % (k, key)
    # the lean per-step launches: the same bits for as long as an environment stays within 32 rows
    lean = runs[("per_step", 1)]
    over = ref["rows"] > A.PACKED_MAXROWS_PER_STEP                           # [T, n]: the step ended above the lean kernel's capacity
    first = np.where(over.any(0), over.argmax(0), T)                         # the first such step of each environment
    # (re-steps by step, cumulative: the three-set launches' own — another capacity, or more than 40 rows — are the lean launches' too; what the lean
    #  launches add beyond the environments seen above 32 rows is an environment that passed 32 rows at an evaluation inside a step: from that step on it
    #  cannot be told apart, and nothing is compared)
    explained = ref["redo_steps"] + np.cumsum(over.sum(1))
    assert np.all(lean["redo_steps"] >= np.cumsum(over.sum(1)))
    unexplained = lean["redo_steps"] > explained
    clean = int(unexplained.argmax()) if unexplained.any() else T
    print(case, "lean re-steps", lean["redo_steps"].tolist(), "three-set", ref["redo_steps"].tolist(), "first step above 32 rows", first.tolist(), "compared steps", clean)
    assert clean >= 1, "nothing left to compare: choose other states"
    for e in range(n):
        upto = min(int(first[e]), clean)
        for t in range(upto):
            assert np.array_equal(lean["obs"][t, e], ref["obs"][t, e]), "env %d (%d rows) differs between the lean and the three-set per-step launches at step %d" % (e, ne0[e], t)
        if upto == T:
            for k in ("qpos", "qvel", "qacc", "solver_iter", "nefc"):
                assert np.array_equal(lean[k][e], ref[k][e]), (k, e)
