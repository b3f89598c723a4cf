"""The cases, the reference-only selection and the error envelope of the float32 library (tests/test_gpu_float32.py) — TEST INFRASTRUCTURE,
numpy and the two CPU oracle builds only (oracle/dm_oracle.c as liboracle.so, float64, and liboracle32.so, the same code in float32).

CASES.  Set A is `H.varied_states(256, seed=31)` with normalised quaternions and actions `RandomState(2).randn(T, n, 28) * 0.5`, T = 3 steps in
lock step with no resynchronisation (the set of test_float32_batch_tracks_the_float64_path); the stage-by-stage comparison evaluates the same
states once with that draw's warm start and ctrl.  Everything is rounded to float32 first: every oracle run sees the numbers the float32
kernels see, and the float64 oracle on those inputs is the REFERENCE.  The small sets n1, n4, n5, n13 are envs of A (an env's results do not
depend on its batch): a lone wave; one full three-wave workgroup plus one wave of the float one-env kernel; partial packed slots.  Each holds an
env of 33 .. 40 rows (the three-row-set solve) beside lighter ones, picked by the reference's row counts alone.

SELECTION.  An env's discrete outcomes (nefc, ncon, the contact geom list, done, frame index and cycle, and the largest row / limit row count over a
step's four RK evaluations) are asserted at step t when the
float64 oracle, the float32 oracle and N_DRAWS float64 runs with every input perturbed by relative 1e-5 (84 float32 ulps; full size, seeded
signs; the root position by absolute 1e-5; the quaternion renormalised) agree on them at t and at every step before it (step 0: the
evaluation of the initial state).  Nothing the kernels compute enters; at most MAX_UNSELECTED of a set may fall outside, and every selected env
is then asserted with no further exclusion.

ENVELOPE.  For a quantity X after step t, e32 = H.rel_err(oracle32, oracle64) per selected env.  The kernels must satisfy, per quantity and
step, max over envs of rel_err(kernel32, oracle64) <= MARGIN * max over envs of e32 and median <= MARGIN * median.  MARGIN = 4 is this
suite's precedent for float32 envelopes (tests/test_gpu_learner_edges.py); a margin at all because two correct float32 evaluations of one
formula differ in summation order, FMA contraction (the oracle is built with -ffp-contract=off) and libm, and the envelope's own p99-to-max
spread on A is a factor of 3.  A small set's max bar is A's (the extreme of 1 .. 13 envs is one draw of A's distribution, not an envelope);
its median bar, from 13 envs up, is its own.  A bar of exactly zero (the alive reward: 1.0 in every build) asks for equality.

MEASURED (this commit, gcc -O2 -ffp-contract=off, glibc libm): median / max of e32 over the selected envs, rollout of set A

    quantity         step 1               step 2               step 3
    obs              3.14e-07 / 4.34e-06  3.85e-07 / 2.71e-06  4.51e-07 / 3.72e-06
    reward (mode 3)  4.43e-08 / 4.50e-07  4.37e-08 / 4.97e-07  5.15e-08 / 4.46e-07
    qpos             4.60e-08 / 1.76e-07  6.27e-08 / 4.40e-07  8.85e-08 / 7.05e-07
    qvel             3.90e-07 / 9.81e-06  4.44e-07 / 6.03e-06  5.17e-07 / 5.41e-06
    qacc_warmstart   1.59e-06 / 2.24e-05  2.05e-06 / 2.73e-05  1.93e-06 / 5.19e-05

and of one evaluation of A's states (the stages of H.compare_forward)

    M 1.33e-07 / 4.45e-07   qfrc_bias 1.38e-07 / 2.15e-06   qacc_smooth 1.80e-06 / 1.90e-05   xipos 9.32e-08 / 1.90e-07
    efc_J 1.00e-07 / 2.23e-06   efc_pos 3.33e-08 / 1.87e-07   efc_R 1.70e-08 / 8.98e-06   efc_aref 1.36e-07 / 2.74e-05
    efc_b 1.80e-07 / 8.81e-06   efc_force 5.10e-07 / 2.24e-05   qacc 1.20e-06 / 1.90e-05

(`RECORDED` below holds every figure, per case set.)  The obs maximum after one step, 4.34e-6, is the figure of a scratch build with `double`
redefined to `float`: the typedef build is the same evaluation.  obs p99 is 1.4e-6 / 1.9e-6 / 2.8e-6.  All 256 envs are selected at the initial evaluation
and after one step, 255 after two and three; the float32 oracle's PGS sweep count equals the float64 oracle's on 252 .. 256 of 256 evaluations (printed
by the tests, not asserted).  By an env's largest reference row count over every RK evaluation: 16 with none, 182 with 1-16, 38 with 17-32, 9 with 33-40, 5 with 41-48,
6 with 49-63; 64 envs raise `done` within the three steps."""
import functools

import numpy as np

from tests import helpers as H

N, T = 256, 3
N_DRAWS, REL_PERTURB = 6, 1e-5
MAX_UNSELECTED = 0.02
MARGIN = 4.0
MAX_EFC = 63                                        # the one-env kernel's capacity, mirrored by the oracle (H.oracle_model)
ROLLOUT_Q = ("obs", "reward", "qpos", "qvel", "qacc_warmstart")
STAGE_Q = ("M", "qfrc_bias", "qacc_smooth", "efc_J", "efc_pos", "efc_R", "efc_aref", "efc_b", "efc_force", "qacc", "xipos")
DISCRETE = ("nefc", "ncon", "geoms", "done", "done_alive", "frame", "cycle", "peak", "limit_peak")
MAXCON = 63

f64r = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # the float32-rounded numbers, as float64


@functools.lru_cache(maxsize=None)
def imitation():
    """(table [F,112], params [32]) of the walk clip, rounded to float32: what Batch(imitation=...) of a dtype=32 batch holds."""
    from deepmimic_mujoco_amd.imitation import ImitationSpec
    tab, par = ImitationSpec(H.compiled_model()).table_for(H.mocap())
    return f64r(tab), f64r(par)


@functools.lru_cache(maxsize=None)
def inputs():
    """Set A's inputs (do not modify): idx [N], q, v, the stage evaluation's ws and ctrl, the rollout's actions [T, N, 28]."""
    idx, q, v, ws, ctrl = H.varied_states(N, seed=31)
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    acts = np.random.RandomState(2).randn(T, N, 28) * 0.5
    return dict(idx=idx, q=f64r(q), v=f64r(v), ws=f64r(ws), ctrl=f64r(ctrl), acts=f64r(acts))


def _perturbed(c, draw):
    """Every input times (1 +- 1e-5), seeded signs; the root position +- 1e-5 absolute; the quaternion renormalised."""
    rng = np.random.RandomState(7000 + draw)
    sgn = lambda a: REL_PERTURB * rng.choice([-1.0, 1.0], size=a.shape)
    q = c["q"] * (1 + sgn(c["q"])); q[:, :3] = c["q"][:, :3] + sgn(c["q"][:, :3])
    q[:, 3:7] /= np.linalg.norm(q[:, 3:7], axis=1, keepdims=True)
    return dict(c, q=q, v=c["v"] * (1 + sgn(c["v"])), acts=c["acts"] * (1 + sgn(c["acts"])))


def _discrete_of(d):
    g = np.full((MAXCON, 2), -1, dtype=np.int32)
    cg = d.get("contact_geom", 4 * MAXCON).reshape(-1, 2).astype(np.int32)[:MAXCON]
    g[:len(cg)] = cg
    return int(d.get("nefc", 1)[0]), int(d.get("ncon", 1)[0]), g


def _rollout(dtype, c):
    """T lock-step steps of every env of A on the oracle build `dtype`, warm start and time zero, reward mode 3 (the alive reward of mode 0 is 1.0
    and its done flag the height test alone).  Index 0 of the discrete arrays is the evaluation of the initial state, index t the state after step t: nefc,
    ncon and the contact list are those of step t's fourth RK evaluation (what sim.data holds after a step), `peak` / `limit_peak` the largest row / limit
    row count of its four evaluations — what decides whether a packed launch form holds the env-step or hands it to the one-env code."""
    from oracle import oracle as O
    om = O.Model(dtype=dtype); om.set("max_efc", MAX_EFC)
    tab, par = imitation()
    r = dict(obs=np.zeros((T, N, 56)), reward=np.zeros((T, N)), qpos=np.zeros((T, N, 35)), qvel=np.zeros((T, N, 34)), qacc_warmstart=np.zeros((T, N, 34)),
             nefc=np.zeros((T + 1, N), dtype=np.int32), ncon=np.zeros((T + 1, N), dtype=np.int32), geoms=np.zeros((T + 1, N, MAXCON, 2), dtype=np.int32),
             done=np.zeros((T + 1, N), dtype=np.uint8), done_alive=np.zeros((T + 1, N), dtype=np.uint8), frame=np.zeros((T + 1, N), dtype=np.int32),
             cycle=np.zeros((T + 1, N), dtype=np.int32), solver_iter=np.zeros((T + 1, N), dtype=np.int32),
             peak=np.zeros((T + 1, N), dtype=np.int32), limit_peak=np.zeros((T + 1, N), dtype=np.int32))
    d = O.Data(om)
    for e in range(N):
        d.reset(); d.set_state(c["q"][e], c["v"][e])
        r["nefc"][0, e], r["ncon"][0, e], r["geoms"][0, e] = _discrete_of(d)
        r["solver_iter"][0, e] = int(d.get("solver_iter", 1)[0])
        r["peak"][0, e], r["limit_peak"][0, e] = r["nefc"][0, e], int(d.get("nlimit", 1)[0])
        fi, cy = int(c["idx"][e]), 0
        r["frame"][0, e] = fi
        for t in range(T):
            o, rew, dn, fi, cy = O.env_step_imitation(om, d, c["acts"][t, e], 1, tab, par, fi, cy)
            r["obs"][t, e] = o; r["reward"][t, e] = rew
            r["qpos"][t, e] = d.get("qpos", 40); r["qvel"][t, e] = d.get("qvel", 40); r["qacc_warmstart"][t, e] = d.get("qacc_warmstart", 40)
            r["nefc"][t + 1, e], r["ncon"][t + 1, e], r["geoms"][t + 1, e] = _discrete_of(d)
            r["done"][t + 1, e] = dn; r["done_alive"][t + 1, e] = d.is_done(); r["frame"][t + 1, e] = fi; r["cycle"][t + 1, e] = cy
            r["solver_iter"][t + 1, e] = int(d.get("solver_iter", 1)[0])
            r["peak"][t + 1, e], r["limit_peak"][t + 1, e] = int(d.get("nefc_peak", 1)[0]), int(d.get("nlimit_peak", 1)[0])
    return r


def stage_arrays(get, nefc):
    """The stage quantities of one evaluation in the shapes H.compare_forward compares; `get(name)` returns the flat array."""
    return {"M": get("M").reshape(34, 34), "qfrc_bias": get("qfrc_bias"), "qacc_smooth": get("qacc_smooth"), "efc_J": get("efc_J").reshape(-1, 34)[:nefc],
            "efc_pos": get("efc_pos")[:nefc], "efc_R": get("efc_R")[:nefc], "efc_aref": get("efc_aref")[:nefc], "efc_b": get("efc_b")[:nefc],
            "efc_force": get("efc_force")[:nefc], "qacc": get("qacc"), "xipos": get("xipos").reshape(14, 3)}


def _stages(dtype, c):
    """One evaluation of every state of A with the draw's warm start and ctrl: a list of {quantity: array} and the PGS sweep counts."""
    from oracle import oracle as O
    om = O.Model(dtype=dtype); om.set("max_efc", MAX_EFC)
    d = O.Data(om)
    out, it = [], np.zeros(N, dtype=np.int32)
    for e in range(N):
        d.set("qacc_warmstart", c["ws"][e]); d.set("ctrl", c["ctrl"][e]); d.set_state(c["q"][e], c["v"][e])
        out.append(stage_arrays(d.get, int(d.get("nefc", 1)[0])))
        it[e] = int(d.get("solver_iter", 1)[0])
    return out, it


def stats(errs):
    """(median, max) of a per-env error list"""
    e = np.asarray(errs, dtype=np.float64)
    return (float(np.median(e)), float(e.max())) if e.size else (0.0, 0.0)


@functools.lru_cache(maxsize=None)
def reference():
    """Everything the GPU tests compare against, computed once per process from the two oracle builds alone (do not modify):
       ref       the float64 oracle's rollout of A (`_rollout`), o32 the float32 oracle's
       stage     the float64 oracle's stage quantities per env, stage_iter its sweep counts; stage32 the float32 oracle's
       selected  bool [T + 1, N]: env e's discrete outcomes are asserted at step t (0: the initial evaluation)
       e32       {quantity: [T, N] per-env rel_err(oracle32, oracle64)} for the rollout (NaN where not selected),
                 {quantity: [N]} for the stages
       rows_max  [N] an env's largest reference row count over every evaluation of the rollout (all four RK stages of every step)"""
    c = inputs()
    ref, o32 = _rollout(64, c), _rollout(32, c)
    runs = [o32] + [_rollout(64, _perturbed(c, k)) for k in range(N_DRAWS)]
    agree = np.ones((T + 1, N), dtype=bool)
    for r in runs:
        for k in DISCRETE:
            same = ref[k] == r[k]
            agree &= same.reshape(T + 1, N, -1).all(axis=2)
    selected = np.logical_and.accumulate(agree, axis=0)
    e32 = {}
    for k in ROLLOUT_Q:
        e32[k] = np.full((T, N), np.nan)
        for t in range(T):
            for e in np.nonzero(selected[t + 1])[0]:
                e32[k][t, e] = H.rel_err(o32[k][t, e], ref[k][t, e])
    stage, stage_iter = _stages(64, c)
    stage32, stage32_iter = _stages(32, c)
    for k in STAGE_Q:
        e32[k] = np.full(N, np.nan)
        for e in np.nonzero(selected[0])[0]:
            e32[k][e] = H.rel_err(stage32[e][k], stage[e][k])
    return dict(inputs=c, ref=ref, o32=o32, stage=stage, stage_iter=stage_iter, stage32=stage32, stage32_iter=stage32_iter, selected=selected, e32=e32,
                rows_max=ref["peak"].max(axis=0))


def row_class(rows_max):
    """0: no rows, 1: 1-16, 2: 17-32, 3: 33-40 (the three-set path), 4: 41-48 (the re-step's register tier), 5: 49-63 (the overflow strip)"""
    return np.searchsorted([1, 17, 33, 41, 49], rows_max, side="right")


@functools.lru_cache(maxsize=None)
def case_sets():
    """{name: env indices into A}.  The small sets take A's envs in index order from two lists made from the reference's row counts alone — `heavy`:
    33 .. 40 rows at most over every RK evaluation of the rollout, selected at every step; `light`: at most 32 rows, selected — placed so that a heavy env shares its
    packed wave (four consecutive envs) with lighter ones."""
    R = reference()
    sel = R["selected"][T]
    cls = row_class(R["rows_max"])
    few_limits = R["ref"]["limit_peak"].max(axis=0) <= 16          # DM_PACKED_MAXLIMROWS: more limit rows leave the packed path whatever the row count
    heavy = [e for e in range(N) if sel[e] and cls[e] == 3 and few_limits[e]]
    light = [e for e in range(N) if sel[e] and cls[e] <= 2 and few_limits[e]]
    assert len(heavy) >= 4 and len(light) >= 16
    h, l = heavy, light
    return {"A": np.arange(N),
            "n1": np.array([h[0]]),
            "n4": np.array([l[0], h[1], l[1], l[2]]),
            "n5": np.array([l[3], l[4], h[2], l[5], h[3]]),
            "n13": np.array([l[6], h[0], l[7], l[8], l[9], l[10], l[11], l[12], h[1], h[2], l[13], l[14], l[15]])}


def envelope(name="A"):
    """{quantity: [(median, max)] per step} (rollout) and {quantity: (median, max)} (stages) of e32 over the set's selected envs"""
    R = reference()
    ids = case_sets()[name]
    env = {}
    for k in ROLLOUT_Q:
        env[k] = [stats([x for x in R["e32"][k][t, ids] if not np.isnan(x)]) for t in range(T)]
    for k in STAGE_Q:
        env[k] = stats([x for x in R["e32"][k][ids] if not np.isnan(x)])
    return env


def bars(name, quantity, step=None):
    """(median bar or None, max bar) a kernel's per-env errors must stay within for `quantity` (after `step`, 0-based, for the rollout quantities)"""
    own, a = envelope(name)[quantity], envelope("A")[quantity]
    if step is not None:
        own, a = own[step], a[step]
    return (MARGIN * own[0] if len(case_sets()[name]) >= 13 else None), MARGIN * a[1]


def check(name, quantity, errs, step=None, what=""):
    """Asserts the envelope on the per-env errors of the set's selected envs; returns (median, max, median bar, max bar) for the record."""
    med, mx = stats(errs)
    bmed, bmax = bars(name, quantity, step)
    tag = "%s %s%s set %s" % (what, quantity, "" if step is None else " step %d" % (step + 1), name)
    print("%-60s median %.2e (bar %s)  max %.2e (bar %.2e)" % (tag, med, "-" if bmed is None else "%.2e" % bmed, mx, bmax))
    assert mx <= bmax, "%s: max rel err %.3e above %.3e" % (tag, mx, bmax)
    assert bmed is None or med <= bmed, "%s: median rel err %.3e above %.3e" % (tag, med, bmed)
    return med, mx, bmed, bmax


# median / max of e32 per case set as measured at this commit (tests/test_float32_oracle.py holds the live envelope to 1.5 x these)
RECORDED = {'A': {'M': (1.329e-07, 4.453e-07),
       'efc_J': (1e-07, 2.234e-06),
       'efc_R': (1.705e-08, 8.982e-06),
       'efc_aref': (1.358e-07, 2.744e-05),
       'efc_b': (1.797e-07, 8.814e-06),
       'efc_force': (5.104e-07, 2.236e-05),
       'efc_pos': (3.327e-08, 1.874e-07),
       'obs': [(3.142e-07, 4.336e-06), (3.852e-07, 2.714e-06), (4.506e-07, 3.718e-06)],
       'qacc': (1.203e-06, 1.902e-05),
       'qacc_smooth': (1.796e-06, 1.902e-05),
       'qacc_warmstart': [(1.588e-06, 2.24e-05), (2.051e-06, 2.727e-05), (1.926e-06, 5.194e-05)],
       'qfrc_bias': (1.384e-07, 2.146e-06),
       'qpos': [(4.603e-08, 1.758e-07), (6.269e-08, 4.401e-07), (8.85e-08, 7.049e-07)],
       'qvel': [(3.897e-07, 9.806e-06), (4.445e-07, 6.03e-06), (5.174e-07, 5.405e-06)],
       'reward': [(4.426e-08, 4.499e-07), (4.371e-08, 4.972e-07), (5.153e-08, 4.455e-07)],
       'xipos': (9.318e-08, 1.903e-07)},
 'n1': {'M': (1.285e-07, 1.285e-07),
        'efc_J': (2.302e-07, 2.302e-07),
        'efc_R': (3.106e-08, 3.106e-08),
        'efc_aref': (2.921e-07, 2.921e-07),
        'efc_b': (2.915e-07, 2.915e-07),
        'efc_force': (7.887e-07, 7.887e-07),
        'efc_pos': (1.623e-07, 1.623e-07),
        'obs': [(3.403e-07, 3.403e-07), (3.497e-07, 3.497e-07), (4.946e-07, 4.946e-07)],
        'qacc': (1.536e-06, 1.536e-06),
        'qacc_smooth': (2.336e-06, 2.336e-06),
        'qacc_warmstart': [(1.168e-06, 1.168e-06), (4.673e-06, 4.673e-06), (7.626e-07, 7.626e-07)],
        'qfrc_bias': (1.717e-07, 1.717e-07),
        'qpos': [(8.652e-08, 8.652e-08), (7.676e-08, 7.676e-08), (1.1e-07, 1.1e-07)],
        'qvel': [(5.11e-07, 5.11e-07), (3.703e-07, 3.703e-07), (4.946e-07, 4.946e-07)],
        'reward': [(1.309e-09, 1.309e-09), (5.188e-09, 5.188e-09), (4.193e-09, 4.193e-09)],
        'xipos': (1.31e-07, 1.31e-07)},
 'n13': {'M': (1.884e-07, 3.637e-07),
         'efc_J': (1.923e-07, 7.303e-07),
         'efc_R': (1.332e-08, 3.106e-08),
         'efc_aref': (2.066e-07, 5.406e-07),
         'efc_b': (2.849e-07, 7.175e-07),
         'efc_force': (7.887e-07, 2.334e-06),
         'efc_pos': (3.731e-08, 1.623e-07),
         'obs': [(5.006e-07, 1.072e-06), (6.905e-07, 1.206e-06), (8.312e-07, 2.749e-06)],
         'qacc': (1.852e-06, 1.287e-05),
         'qacc_smooth': (2.336e-06, 1.287e-05),
         'qacc_warmstart': [(1.845e-06, 6.353e-06), (2.964e-06, 1.32e-05), (2.094e-06, 1.411e-05)],
         'qfrc_bias': (1.106e-07, 7.322e-07),
         'qpos': [(4.693e-08, 1.738e-07), (8.801e-08, 4.401e-07), (1.1e-07, 7.049e-07)],
         'qvel': [(5.298e-07, 1.821e-06), (9.774e-07, 1.741e-06), (9.663e-07, 5.405e-06)],
         'reward': [(5.492e-08, 3e-07), (2.527e-08, 3.054e-07), (2.531e-08, 3.037e-07)],
         'xipos': (9.265e-08, 1.354e-07)},
 'n4': {'M': (1.386e-07, 1.947e-07),
        'efc_J': (5.309e-08, 1.949e-07),
        'efc_R': (6.662e-09, 3.557e-08),
        'efc_aref': (4.302e-08, 2.066e-07),
        'efc_b': (2.256e-08, 2.016e-07),
        'efc_force': (1.269e-07, 1.269e-06),
        'efc_pos': (4.958e-09, 6.834e-08),
        'obs': [(6.096e-07, 1.057e-06), (6.086e-07, 1.12e-06), (7.723e-07, 1.372e-06)],
        'qacc': (3.683e-06, 4.902e-06),
        'qacc_smooth': (3.451e-06, 4.902e-06),
        'qacc_warmstart': [(2.853e-06, 3.209e-06), (2.305e-06, 3.004e-06), (1.864e-06, 2.993e-06)],
        'qfrc_bias': (1.405e-07, 7.322e-07),
        'qpos': [(7.796e-08, 1.738e-07), (9.489e-08, 4.401e-07), (1.345e-07, 7.049e-07)],
        'qvel': [(1.232e-06, 1.668e-06), (8.962e-07, 1.793e-06), (1.088e-06, 1.657e-06)],
        'reward': [(1.368e-07, 3.325e-07), (1.907e-08, 3.721e-08), (3.573e-08, 1.598e-07)],
        'xipos': (1.204e-07, 1.444e-07)},
 'n5': {'M': (1.352e-07, 2.113e-07),
        'efc_J': (2.394e-07, 5.974e-07),
        'efc_R': (3.106e-08, 3.106e-08),
        'efc_aref': (3.232e-07, 5.538e-07),
        'efc_b': (2.849e-07, 8.652e-07),
        'efc_force': (1.218e-06, 2.663e-06),
        'efc_pos': (3.825e-08, 8.945e-08),
        'obs': [(5.34e-07, 7.899e-07), (5.503e-07, 7.741e-07), (4.133e-07, 1.013e-06)],
        'qacc': (1.598e-06, 1.861e-06),
        'qacc_smooth': (2.402e-06, 1.647e-05),
        'qacc_warmstart': [(2.941e-06, 5.792e-06), (2.431e-06, 4.286e-06), (1.551e-06, 5.302e-06)],
        'qfrc_bias': (1.679e-07, 2.683e-07),
        'qpos': [(4.204e-08, 8.09e-08), (8.76e-08, 1.439e-07), (1.315e-07, 2.448e-07)],
        'qvel': [(5.34e-07, 7.899e-07), (5.545e-07, 1.079e-06), (6.563e-07, 1.491e-06)],
        'reward': [(1.045e-08, 4.499e-07), (2.527e-08, 5.45e-08), (2.531e-08, 7.087e-08)],
        'xipos': (9.574e-08, 1.003e-07)}}
