"""What tests/test_slot_capacities.py (the wave testbench) and tests/test_gpu_slot_capacities.py (the device) share: the waves built from
tests/golden/slot_capacities.npz (tools/make_capacity_golden.py), what dm_batch_redo_total must count for them after one step, and the oracle's four steps.
A plain module: numpy and the oracle only.

Waves put an edge state (entry names ending in _at: at a capacity of the packed row builder; _past: one past it) next to a no-row state, a light state and an
edge state of another capacity.  CASES groups them by what must be counted, since the counters are the batch's, not an environment's:
  one_leaves       three waves, in each one environment past a capacity (limit rows / contact pairs / candidates) and three that stay;
  several_leave    a wave two environments leave for different reasons, a wave all four slots of which are past a capacity, a last wave of two;
  none_leaves      only "at", light and no-row environments — every capacity exactly reached, the second narrow-phase trip at 17, 21 and 32 candidates, a wave whose
                   only environment with 17 or more candidates sits in slot 3 beside partners below 8 — and a last wave of two: nothing may be counted.
36 environments in all."""
import numpy as np

from deepmimic_mujoco_amd import _abi as A
from tests import helpers as H
from tests import rows_numpy as RW

T = 4
CASES = {
    "one_leaves": [["limits_past", "norow", "light_0", "frames_at"],
                   ["light_1", "frames_past", "norow", "candidates_16"],
                   ["norow", "light_2", "limits_at", "candidates_past"]],
    "several_leave": [["frames_past", "norow", "candidates_past", "light_3"],
                      ["limits_past", "frames_past", "candidates_past", "limits_past"],
                      ["frames_past", "limits_at"]],
    "none_leaves": [["norow", "light_4", "light_5", "candidates_17"],
                    ["candidates_20plus", "norow", "light_0", "frames_at"],
                    ["candidates_at", "light_1", "norow", "candidates_16"],
                    ["candidates_at", "limits_at"]],
}
SLOT3_WAVE = ("none_leaves", 0)          # the wave whose only environment with 17 or more candidates sits in slot 3
# the reason an environment one past a capacity is counted under; contacts_past joins when the generator reaches it (it is not placed in a wave: the fixture
# may lack it)
PAST_REASON = {"limits_past": RW.REASON["limits"], "frames_past": RW.REASON["frames"], "candidates_past": RW.REASON["candidates"]}
# the narrow-phase fixtures (leg capsule against foot box, foot box against foot box), stepped once from rest on the packed path.  A pose on a discontinuity
# of the step map — the oracle's own answers split within a 1e-15 neighbourhood of it (tools/fuzz_parity.py's criterion) — would be left out here by index:
# at most one in ten of a file, none of the box-box file.  None is.
NARROW_FILES = ("capsule_box_poses", "capsule_box_deep_poses", "box_box_poses")
NARROW_LEFT_OUT = {"capsule_box_poses": [], "capsule_box_deep_poses": [], "box_box_poses": []}
_FIXTURE = []
_ORACLE = {}


def fixture():
    """{entry name: {frame, qpos, qvel, qacc_warmstart, action, counts {name: n}, peaks {name: n}, late_contacts}}, and the list of unreached edges"""
    if not _FIXTURE:
        g = np.load(H.GOLDEN + "/slot_capacities.npz")
        ent = {}
        for i, name in enumerate(g["name"].tolist()):
            ent[name] = dict(frame=int(g["frame"][i]), qpos=g["qpos"][i], qvel=g["qvel"][i], qacc_warmstart=g["qacc_warmstart"][i], action=g["action"][i],
                             counts=dict(zip(g["count_names"].tolist(), g["counts"][i].tolist())), peaks=dict(zip(g["peak_names"].tolist(), g["peaks"][i].tolist())),
                             late_contacts=int(g["late_contacts"][i]))
        _FIXTURE.append((ent, g["unreached"].tolist()))
    return _FIXTURE[0]


def names_of(case):
    return [n for wave in CASES[case] for n in wave]


def states(case):
    """-> (entry names [n], frame, qpos, qvel, warm start, actions [T, n, 28]: row 0 is the fixture's — the step the recorded maxima belong to)"""
    ent, _u = fixture()
    names = names_of(case)
    pick = lambda k: np.array([ent[n][k] for n in names])
    acts = np.random.RandomState(200 + sorted(CASES).index(case)).randn(T, len(names), 28) * 0.9
    acts[0] = pick("action")
    return names, pick("frame").astype(np.int32), pick("qpos"), pick("qvel"), pick("qacc_warmstart"), acts


def expected_reasons(names):
    """dm_batch_redo_total's six counters after ONE step of these environments: every "past" environment under its reason, exactly once; nothing else"""
    want = [0] * 6
    for n in names:
        if n in PAST_REASON:
            want[0] += 1; want[PAST_REASON[n]] += 1
    return want


def oracle(case):
    """the oracle's T steps, computed once per case and read-only: obs [T, n, 56], done [T, n], and after every step nefc [T, n], ncon [T, n] and the contacts'
    geoms [T, n, MAXEFC, 2] (-1 beyond the list), as DM_F_NEFC / DM_F_NCON / DM_F_CONTACT_GEOMS hold them"""
    if case not in _ORACLE:
        from oracle import oracle as O
        _names, _f, q, v, ws, acts = states(case)
        om = H.oracle_model()
        n = len(q)
        out = dict(obs=np.zeros((T, n, 56)), done=np.zeros((T, n), dtype=np.uint8), nefc=np.zeros((T, n), dtype=np.int32), ncon=np.zeros((T, n), dtype=np.int32),
                   geoms=np.full((T, n, A.MAXEFC, 2), -1, dtype=np.int32))
        for e in range(n):
            od = O.Data(om); od.reset(); od.set("qacc_warmstart", ws[e]); od.set_state(q[e], v[e])
            for t in range(T):
                o, _r, d, _ = od.env_step(acts[t, e])
                nc = int(od.get("ncon")[0]); k = min(nc, A.MAXEFC)
                out["obs"][t, e] = o; out["done"][t, e] = d; out["nefc"][t, e] = int(od.get("nefc")[0]); out["ncon"][t, e] = nc
                out["geoms"][t, e, :k] = od.get("contact_geom").reshape(-1, 2)[:k]
        for x in out.values():
            x.setflags(write=False)
        _ORACLE[case] = out
    return _ORACLE[case]


def narrow_poses():
    """-> (file of each pose, qpos [n, 35]): the three files' poses but the ones left out, in file order"""
    files, qs = [], []
    for name in NARROW_FILES:
        q = np.load(H.GOLDEN + "/%s.npy" % name)
        left = NARROW_LEFT_OUT[name]
        assert len(left) * 10 <= len(q) and not NARROW_LEFT_OUT["box_box_poses"], "at most one pose in ten of a file may be left out, none of the box-box file"
        for i in range(len(q)):
            if i not in left:
                files.append(name); qs.append(q[i])
    return files, np.array(qs)


def narrow_oracle():
    """one oracle step of every narrow-phase pose from rest under a zero action (once, read-only): obs, done, nefc, ncon, geoms as oracle() gives them, and
    `inside` [n]: every count of the step's four evaluations stays inside the packed path's capacities (rows: the lean kernel's 32; candidates, counted at the
    pose only: at most 30) — such a pose may not be handed to the one-env code"""
    if "narrow" not in _ORACLE:
        from oracle import oracle as O
        _files, qs = narrow_poses()
        cm = H.compiled_model()
        n = len(qs)
        out = dict(obs=np.zeros((n, 56)), done=np.zeros(n, dtype=np.uint8), nefc=np.zeros(n, dtype=np.int32), ncon=np.zeros(n, dtype=np.int32),
                   geoms=np.full((n, A.MAXEFC, 2), -1, dtype=np.int32), inside=np.zeros(n, dtype=bool))
        od = O.Data(H.oracle_model())
        for e in range(n):
            c = RW.counts_at(cm, od, qs[e], np.zeros(34), np.zeros(34))
            o, d, pk = RW.step_maxima(od, np.zeros(28))
            nc = int(od.get("ncon")[0]); k = min(nc, A.MAXEFC)
            out["obs"][e] = o; out["done"][e] = d; out["nefc"][e] = int(od.get("nefc")[0]); out["ncon"][e] = nc
            out["geoms"][e, :k] = od.get("contact_geom").reshape(-1, 2)[:k]
            out["inside"][e] = all(pk[x] <= RW.CAPS[x] for x in pk) and all(c[x] <= RW.CAPS[x] for x in RW.CAPS) and c["candidates"] <= 30
        for x in out.values():
            x.setflags(write=False)
        _ORACLE["narrow"] = out
    return _ORACLE["narrow"]


def rel_err(got, want):
    """the suite's relative error of an observation block, env by env -> [..., n]"""
    return np.abs(got - want).max(axis=-1) / np.maximum(1.0, np.abs(want).max(axis=-1))
