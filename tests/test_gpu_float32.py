"""The float32 library (libdmenv32.so, Batch(dtype=32)) held to the CPU oracle env by env on every launch form.  The reference is the float64 oracle on
the float32-rounded inputs; the bars are 4 x the error of the float32 build of the same oracle (tests/float32_cases.py: cases, reference-only selection,
envelope — checked on the CPU by tests/test_float32_oracle.py).  The float64 batch is not a reference here.  Every figure is printed before it is
asserted (pytest -s)."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch
from tests import float32_cases as F
from tests import helpers as H
from tests import gpu_batch as GB
from tests.gpu_batch import horizon_rows

pytestmark = pytest.mark.gpu
T = F.T

# this file's launch-form ids -> tests/gpu_batch.py FORMS ("horizon": dm_batch_rollout, T steps in one launch, re-steps inside the wave)
FORMS = {"narrow": "narrow", "narrow-pipe2": "narrow-pipe2", "packed": "packed", "packed-ext": "packed-ext", "horizon": "rollout", "queue": "queue-3"}
IN_WAVE = ("packed-ext", "horizon", "queue")            # forms whose packed code holds DM_PACKED_MAXROWS = 40 rows
SETS = ("A", "n1", "n4", "n5", "n13")


def make(n, mode=0):
    mc = H.mocap()
    b = Batch(H.compiled_model(), mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt), imitation=F.imitation(), dtype=32)
    b.set_option(A.OPT_REWARD_MODE, mode)
    return b


def start_envs(b, ids):
    c = F.inputs()
    GB.start(b, c["idx"][ids], c["q"][ids], c["v"][ids])


def physics_of(b):
    return dict(qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL), qacc_warmstart=b.get(A.F_QACC_WARMSTART), nefc=b.get(A.F_NEFC), ncon=b.get(A.F_NCON),
                geoms=b.get(A.F_CONTACT_GEOMS)[:, :F.MAXCON], frame=b.get(A.F_FRAME_IDX), cycle=b.get(A.F_CYCLE), time=b.get(A.F_TIME))


def run_form(form, ids, mode, acts=None, per_step_state=True):
    """T lock-step steps of the envs `ids` of set A through one launch form -> rows (obs, reward, done as numpy), the state after every step where the
    form lets it be read between steps (else only the last: a list with None before it), the initial evaluation's counts, the redo counters."""
    lf = GB.FORMS[FORMS[form]]
    n = len(ids)
    acts = F.inputs()["acts"][:, ids] if acts is None else acts
    steps = acts.shape[0]
    b = make(n, mode)
    b.set_option(A.OPT_PACKED, lf.packed); b.set_option(A.OPT_PIPELINE, lf.pipeline)
    start_envs(b, ids)
    first = dict(nefc=b.get(A.F_NEFC), ncon=b.get(A.F_NCON), geoms=b.get(A.F_CONTACT_GEOMS)[:, :F.MAXCON])
    ac, ob, rew, dn, _vp = horizon_rows(steps, n, act=acts)
    states = []
    queue = lf.issue == "queue"

    def read_state(_t):
        b.join(); b.sync()
        states.append(physics_of(b))
    GB.issue_steps(b, lf, ac, ob, rew, dn, 1, between=read_state if per_step_state and not queue else None)
    if len(states) < steps:
        states = [None] * (steps - 1) + [physics_of(b)]
    qs = b.queue_stats() if queue else None
    redo = b.redo_reasons()
    b.close()
    if queue:
        assert qs[:2] == (1, steps), "the %d queued steps must run as one horizon launch %s" % (steps, qs)
    return dict(obs=ob.cpu().numpy(), reward=rew.cpu().numpy(), done=dn.cpu().numpy(), states=states, first=first, redo=redo)


def assert_discrete(out, ids, mode, what):
    """done after every step; nefc, ncon, the contact list (and in mode 3 the frame index and cycle) wherever the form shows the state: exactly the
    reference's on every selected env"""
    R = F.reference()
    ref, sel = R["ref"], R["selected"][:, ids]
    for k in ("nefc", "ncon", "geoms"):
        s = sel[0]
        assert np.array_equal(out["first"][k][s], ref[k][0][ids][s]), "%s: %s of the initial evaluation" % (what, k)
    for t in range(T):
        s = sel[t + 1]
        assert np.array_equal(out["done"][t][s], ref["done" if mode == 3 else "done_alive"][t + 1][ids][s]), "%s: done after step %d" % (what, t + 1)
        st = out["states"][t]
        if st is None:
            continue
        for k in ("nefc", "ncon", "geoms") + (("frame", "cycle") if mode == 3 else ()):
            assert np.array_equal(st[k][s], ref[k][t + 1][ids][s]), "%s: %s after step %d" % (what, k, t + 1)


def assert_envelope(out, name, ids, mode, what):
    """obs and reward after every step, qpos / qvel / qacc_warmstart wherever the form shows the state, against the float64 oracle within the envelope"""
    R = F.reference()
    ref, sel = R["ref"], R["selected"][:, ids]
    rows = []
    for t in range(T):
        s = np.nonzero(sel[t + 1])[0]
        rows.append(("obs", t) + F.check(name, "obs", [H.rel_err(out["obs"][t, e], ref["obs"][t, ids[e]]) for e in s], t, what))
        if mode == 3:
            rows.append(("reward", t) + F.check(name, "reward", [H.rel_err(out["reward"][t, e], ref["reward"][t, ids[e]]) for e in s], t, what))
        else:
            assert np.all(out["reward"][t] == 1.0), "%s: the alive reward is 1.0" % what
        st = out["states"][t]
        if st is not None:
            for k in ("qpos", "qvel", "qacc_warmstart"):
                rows.append((k, t) + F.check(name, k, [H.rel_err(st[k][e], ref[k][t, ids[e]]) for e in s], t, what))
    return rows


def row_redo_counts(ids):
    """From the reference alone, over the selected env-steps of the envs `ids`: (n32, n40, sure, slack).  n32 / n40: env-steps some RK evaluation of which holds
    more than 32 / 40 rows (or more than DM_PACKED_MAXLIMROWS limit rows): what a packed form holding 32 / 40 rows must hand to the one-env code for ROWS.
    sure: env-steps of 33 .. 40 rows that BEGIN above 32 — a horizon launch picks a wave-step's instantiation from the row counts the step before left
    (slot_step.h slot_rollout), so these run the three-set code for certain, while one that jumps there from fewer rows may be re-stepped.  slack: the
    unselected env-steps, whose counts the reference does not vouch for."""
    ref, sel = F.reference()["ref"], F.reference()["selected"]
    n32 = n40 = sure = slack = 0
    for t in range(T):
        s_ = sel[t + 1][ids]
        lim = ref["limit_peak"][t + 1][ids] > A.PACKED_MAXLIMROWS
        pk = ref["peak"][t + 1][ids]
        n32 += int((((pk > A.PACKED_MAXROWS_PER_STEP) | lim) & s_).sum()); n40 += int((((pk > A.PACKED_MAXROWS) | lim) & s_).sum())
        sure += int(((pk > A.PACKED_MAXROWS_PER_STEP) & (pk <= A.PACKED_MAXROWS) & ~lim & (ref["nefc"][t][ids] > A.PACKED_MAXROWS_PER_STEP) & s_).sum())
        slack += int((~s_).sum())
    return n32, n40, sure, slack


def may_jump(ids):
    """[len(ids)] bool, from the reference: the env has a step of 33 .. 40 rows that begins with at most 32 — the one case in which a horizon launch and the
    per-step launches with the three-set code may solve the same env-step with different code (the wave's lean instantiation, then the in-wave re-step)."""
    ref = F.reference()["ref"]
    pk, before = ref["peak"][1:, ids], ref["nefc"][:T, ids]
    return ((pk > A.PACKED_MAXROWS_PER_STEP) & (pk <= A.PACKED_MAXROWS) & (before <= A.PACKED_MAXROWS_PER_STEP)).any(axis=0)


# ---- 1. the one-env kernel, stage by stage ------------------------------------------------------------------------------------------------
def test_one_env_kernel_stage_by_stage():
    """Batch.debug_forward (DM_OPT_PACKED 0) on set A with the draw's warm start and ctrl: M, qfrc_bias, qacc_smooth, the constraint rows, the solved forces,
    qacc and xipos within the stage envelope; nefc, ncon and the contact list exact on every selected env.  PGS sweep counts: printed."""
    R = F.reference()
    c, sel = R["inputs"], R["selected"][0]
    b = make(F.N); b.set_option(A.OPT_PACKED, 0)
    b.set(A.F_QACC_WARMSTART, c["ws"]); b.set(A.F_CTRL, c["ctrl"])
    b.set_state(c["q"], c["v"], frame_idx=c["idx"])
    cg = b.get(A.F_CONTACT_GEOMS)[:, :F.MAXCON]
    errs = {k: [] for k in F.STAGE_Q}
    it_same = 0
    for e in np.nonzero(sel)[0]:
        dbg = b.debug_forward(int(e))
        assert dbg["nefc"] == R["ref"]["nefc"][0, e] and dbg["ncon"] == R["ref"]["ncon"][0, e], (e, dbg["nefc"], dbg["ncon"])
        assert np.array_equal(cg[e], R["ref"]["geoms"][0, e]), "contact (geom1, geom2) list of env %d" % e
        it_same += int(dbg["solver_iter"] == R["stage_iter"][e])
        got = F.stage_arrays(lambda k: np.asarray(dbg[k]), dbg["nefc"])
        for k in F.STAGE_Q:
            errs[k].append(H.rel_err(got[k], R["stage"][e][k]))
    b.close()
    print("PGS sweep count equals the float64 oracle's on %d of %d envs (the float32 oracle's: %d)" %
          (it_same, int(sel.sum()), int((R["stage_iter"] == R["stage32_iter"])[sel].sum())))
    for k in F.STAGE_Q:
        F.check("A", k, errs[k], None, "stage")


# ---- 2. every launch form, three lock-step steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_launch_form_three_steps(form, mode):
    """obs, reward and (where the form shows it: after every per-step launch, else after the last step) qpos / qvel / qacc_warmstart within the envelope; done,
    nefc, ncon, contact lists and frame indices exact on the selected envs; the redo counters say that 33 .. 40-row envs were re-stepped by the redo
    kernel on DM_OPT_PACKED 1 and stayed in their wave on DM_OPT_PACKED 2, in the horizon launch and in the step queue, and that envs above 40 rows
    were re-stepped everywhere."""
    for name in SETS:
        ids = F.case_sets()[name]
        what = "%s mode %d" % (form, mode)
        out = run_form(form, ids, mode)
        assert np.isfinite(out["obs"]).all()
        assert_discrete(out, ids, mode, what + " set " + name)
        assert_envelope(out, name, ids, mode, what)
        redo = out["redo"]
        print("%s set %s: redo [total, candidates, box slots, contacts, rows, PGS test] %s" % (what, name, redo))
        if GB.FORMS[FORMS[form]].packed == 0:
            assert redo[0] == 0
            continue
        n32, n40, sure, slack = row_redo_counts(ids)
        print("%s set %s: env-steps above 32 rows %d, above 40 rows %d, 33 .. 40 rows from above 32: %d" % (what, name, n32, n40, sure))
        assert n32 > n40, "set %s holds no env-step of 33 .. 40 rows" % name
        if form == "packed":                      # everything above 32 rows through the redo kernel
            assert n32 <= redo[4] <= n32 + slack, (what, name, redo, n32)
        elif form == "packed-ext":                # 33 .. 40 rows stay in the wave, above 40 re-stepped
            assert n40 <= redo[4] <= n40 + slack, (what, name, redo, n40)
        else:                                     # horizon launch, step queue: the same, except an env-step that jumps to 33 .. 40 rows from at most 32
            assert n40 <= redo[4] <= n32 - sure + slack, (what, name, redo, n40, n32, sure)
        if name == "A":
            assert n40 > 0 and sure > 0


# ---- 3. the packed forms agree bit for bit in float32 too --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3])
def test_packed_forms_are_bit_identical(mode):
    """per-step packed, horizon launch and step queue from the same state give the same bits — obs, reward, done of every step and the final
    state.  The step queue on EVERY env of A; the per-step launches with the three-set code (DM_OPT_PACKED 2) on every env but those with a step that jumps to
    33 .. 40 rows from at most 32 (`may_jump`); the lean per-step kernel (DM_OPT_PACKED 1) on the envs that never hold more than its 32 rows in any RK
    evaluation (the reference's peak counts) — above it that form re-steps with the one-env code what the others solve in the wave."""
    ids = F.case_sets()["A"]
    outs = {form: run_form(form, ids, mode, per_step_state=False) for form in ("packed", "packed-ext", "horizon", "queue")}
    keys = ("qpos", "qvel", "qacc_warmstart", "nefc", "ncon", "geoms", "frame", "cycle", "time")

    def differing(x, y):
        bad = np.zeros(len(ids), dtype=bool)
        for k in ("obs", "reward", "done"):
            bad |= (x[k] != y[k]).reshape(T, len(ids), -1).any(axis=(0, 2))
        for k in keys:
            bad |= (x["states"][-1][k] != y["states"][-1][k]).reshape(len(ids), -1).any(axis=1)
        return bad

    ref, R = outs["horizon"], F.reference()
    light = (R["rows_max"][ids] <= A.PACKED_MAXROWS_PER_STEP) & (R["ref"]["limit_peak"][:, ids].max(axis=0) <= A.PACKED_MAXLIMROWS)
    same_code = {"queue": np.ones(len(ids), dtype=bool), "packed-ext": ~may_jump(ids), "packed": light}
    assert light.sum() > 200 and same_code["packed-ext"].sum() > 240
    fails = []
    for form in ("queue", "packed-ext", "packed"):
        bad = differing(outs[form], ref)
        print("mode %d: %s against the horizon launch: %d of %d envs differ, %d of the %d envs both forms step with the same code" %
              (mode, form, int(bad.sum()), len(ids), int((bad & same_code[form]).sum()), int(same_code[form].sum())))
        if (bad & same_code[form]).any():
            fails.append("%s differs from the horizon launch on envs %s" % (form, np.nonzero(bad & same_code[form])[0][:10]))
    assert not fails, fails


# ---- 4. who shares the wave does not matter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed-ext", "horizon"])
def test_wave_partners_do_not_matter(form):
    """A <= 32-row env's results are bit-identical whether its wave partners are light or 33 .. 40-row envs (its wave then runs the three-set instantiation;
    the light env's surplus terms are exact zeros), as tests/test_wave_testbench.py asserts for float64."""
    R = F.reference()
    ids = F.case_sets()["n13"].copy()
    cls = F.row_class(R["rows_max"])
    heavy_at = np.nonzero(cls[ids] == 3)[0]
    spare = [e for e in range(F.N) if cls[e] <= 2 and R["selected"][T, e] and R["ref"]["limit_peak"][:, e].max() <= A.PACKED_MAXLIMROWS and e not in set(ids.tolist())]
    assert len(heavy_at) >= 3 and len(spare) >= len(heavy_at)
    alone = ids.copy(); alone[heavy_at] = spare[:len(heavy_at)]
    assert (cls[alone] <= 2).all() and {int(p) // 4 for p in heavy_at} >= {0, 2}            # heavy envs in two of the four waves
    for mode in (0, 3):
        x, y = run_form(form, ids, mode, per_step_state=False), run_form(form, alone, mode, per_step_state=False)
        assert y["redo"][4] == 0 and x["redo"][4] <= row_redo_counts(ids)[0] - row_redo_counts(ids)[2]
        keep = np.array([p for p in range(len(ids)) if p not in set(heavy_at.tolist())])
        for k in ("obs", "reward", "done"):
            assert np.array_equal(x[k][:, keep], y[k][:, keep]), (form, mode, k)
        for k in ("qpos", "qvel", "qacc_warmstart", "nefc", "frame"):
            assert np.array_equal(x["states"][-1][k][keep], y["states"][-1][k][keep]), (form, mode, k)


# ---- 5. the float-only policy branch of the horizon launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 64])
def test_horizon_with_policy_replays_open_loop_bit_for_bit(n):
    """kernels_rollout.hip: the policy step's scratch runs into a float32 slot's kinematics, so a step that follows a policy step must recompute them
    (kin_carry off).  A T = 8 horizon with a seeded MlpPolicy inside, then the actions it recorded replayed open loop through a horizon launch without a
    policy (which carries the kinematics from step to step in mode 3): obs, reward, done and the final state must be the same bits.  The first step's obs,
    whose action is the caller's, also meet the envelope against the oracle."""
    R = F.reference()
    ids = F.case_sets()["n13"] if n == 13 else np.arange(64)
    TT = 8
    c = F.inputs()
    pol, W = GB.fused_policy()
    for mode in (3, 0):
        res = []
        acts = None
        for with_policy in (True, False):
            b = make(n, mode); b.set_option(A.OPT_PACKED, 1)
            start_envs(b, ids)
            ac, ob, rew, dn, vp = horizon_rows(TT, n, a0=c["acts"][0, ids])
            if not with_policy:
                ac[:] = acts
            b.rollout(ac, (ob, rew, dn), 1, W if with_policy else None, vp if with_policy else None, True, pol._seed, 7)
            b.join(); b.sync()
            if with_policy:
                acts = ac.clone()
                assert bool(torch.isfinite(acts).all()) and float(acts[1:].abs().max()) > 0, "the policy wrote no actions"
            res.append((ob.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy(), physics_of(b)))
            b.close()
        (o1, r1, d1, s1), (o2, r2, d2, s2) = res
        assert np.isfinite(o1).all()
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2), "mode %d: the replay differs in step %s" % (
            mode, np.nonzero((o1 != o2).any(axis=(1, 2)))[0][:3])
        for k in s1:
            assert np.array_equal(s1[k], s2[k]), (mode, k)
        s = np.nonzero(R["selected"][1, ids])[0]
        F.check("n13" if n == 13 else "A", "obs", [H.rel_err(o1[0, e], R["ref"]["obs"][0, ids[e]]) for e in s], 0, "horizon with policy, mode %d, n %d" % (mode, n))


# ---- 6. auto-reset inside a float32 horizon ----------------------------------------------------------------------------------------------------
def test_autoreset_inside_a_horizon_lands_on_the_rounded_mocap_frame():
    """RSI auto-reset (DM_OPT_AUTORESET 1) inside a horizon launch of 64 envs, reward mode 3: the observation row of a step that ended an episode is the fresh
    episode's — the mocap frame reset_env draws for (seed, env, episode), rounded to float32, exactly; an env reset by the last step holds that frame in qpos /
    qvel; and the step after a reset, from that state with a zero warm start, meets the envelope against the float64 oracle (bars: 4 x A's first-step
    maxima, 4 x the float32 oracle's own median on these very steps)."""
    from oracle import oracle as O
    n, TT, seed = 64, 6, 11
    mc = H.mocap(); Fr = mc.data_config.shape[0]
    tab, par = F.imitation()
    ids = np.arange(n)
    acts = F.f64r(np.random.RandomState(12).randn(TT, n, 28) * 0.5)
    b = make(n, 3); b.set_option(A.OPT_PACKED, 1); b.set_option(A.OPT_AUTORESET, 1); b.set_option(A.OPT_SEED, seed)
    start_envs(b, ids)
    ep = b.get(A.F_EPISODE).copy()
    ac, ob, rew, dn, _vp = horizon_rows(TT, n, act=acts)
    b.rollout(ac, (ob, rew, dn), 1)
    b.join(); b.sync()
    ob, rew, dn = ob.cpu().numpy(), rew.cpu().numpy(), dn.cpu().numpy()
    final = physics_of(b); ep_end = b.get(A.F_EPISODE)
    b.close()
    assert np.isfinite(ob).all() and dn.any(axis=0).sum() >= 0.1 * n, "%d of %d envs reset" % (int(dn.any(axis=0).sum()), n)
    oms = {64: O.Model(dtype=64), 32: O.Model(dtype=32)}
    for m in oms.values():
        m.set("max_efc", F.MAX_EFC)
    e_obs, e_rew, e32_obs, e32_rew = [], [], [], []
    for e in range(n):
        for t in np.nonzero(dn[:, e])[0]:
            k = H.device_rsi_frame(seed, e, int(ep[e]), Fr); ep[e] += 1
            q0, v0 = F.f64r(mc.data_config[k]), F.f64r(mc.data_vel[k])
            assert np.array_equal(ob[t, e], np.concatenate([q0[7:], v0[6:]])), "env %d step %d: not the rounded mocap frame %d" % (e, t, k)
            if t == TT - 1:
                assert np.array_equal(final["qpos"][e], q0) and np.array_equal(final["qvel"][e], v0) and final["frame"][e] == k and final["cycle"][e] == 0
                assert final["time"][e] == 0 and not final["qacc_warmstart"][e].any()
            elif not dn[t + 1, e]:
                got = {}
                for dt, om in oms.items():
                    d = O.Data(om); d.reset(); d.set_state(q0, v0)
                    got[dt] = O.env_step_imitation(om, d, acts[t + 1, e], 1, tab, par, k, 0)
                assert bool(got[64][2]) is False
                e_obs.append(H.rel_err(ob[t + 1, e], got[64][0])); e_rew.append(H.rel_err(rew[t + 1, e], got[64][1]))
                e32_obs.append(H.rel_err(got[32][0], got[64][0])); e32_rew.append(H.rel_err(got[32][1], got[64][1]))
    assert np.array_equal(ep, ep_end)
    assert len(e_obs) >= 5, "too few steps after a reset inside the horizon (%d)" % len(e_obs)
    for name, errs, own in (("obs", e_obs, e32_obs), ("reward", e_rew, e32_rew)):
        (med, mx), (omed, omx) = F.stats(errs), F.stats(own)
        bmax = F.bars("A", name, 0)[1]
        print("step after a reset, %s over %d env-steps: median %.2e (float32 oracle %.2e)  max %.2e (float32 oracle %.2e, bar %.2e)" % (name, len(errs), med, omed, mx, omx, bmax))
        assert mx <= bmax
        assert len(errs) < 13 or med <= F.MARGIN * omed
