#!/usr/bin/env python3
"""Record tests/golden/slot_capacities.npz: states that sit AT and ONE PAST each per-environment capacity of the packed step's row builder (csrc/slot_kernel.h
slot_rows; include/dmenv.h DM_PACKED_*), with the partners that fill their waves.  Only the CPU oracle and tests/rows_numpy.py are used: nothing here runs the
kernels, so the file says where the edges are, not what the kernels do there.

Edges (entry names): limits_at / limits_past (16 / 17 limit rows), frames_at / frames_past (8 / 9 geom pairs with a contact), contacts_at / contacts_past (13 /
14 contacts), candidates_16 / candidates_17 (one narrow-phase trip / two), candidates_20plus, candidates_at / candidates_past (32 / 33 broad-phase candidates);
partners: norow, light_0 .. light_5 (1 .. 11 rows, fewer than 8 candidates).

An "at" state: its own count equals the capacity at the state and the largest of the step's four evaluations (the oracle's *_peak fields) is still the capacity;
every other count, and the rows (at most 32), stay inside their capacities over the whole step.  A "past" state: at the state only its own count is past its
capacity, rows at most 32.  The oracle has no broad phase, so candidates are counted by numpy at the state only; every state that is not a candidate edge keeps
two away from the trip edge (at most 14, or 19 .. 30).  A state whose entry speaks of the second trip (candidates_17, _20plus, _at) holds a contact among
the candidates 16 and up: skipping the second trip loses a row.

Sources, in this order: the constructed limit poses (qpos0 with the root at z = 3 and the first k limited hinges 0.02 rad past alternating bounds); oracle
rollouts past falls under N(0, 0.9^2) actions on every bundled clip; the lying and deep poses tools/fuzz_parity.py builds; a curled pose in the air, climbed
joint by joint (inside the joint ranges) towards 32 and 33 candidates with at most 8 contact pairs.  The first state met per entry is kept.

    python3 tools/make_capacity_golden.py [--out tests/golden/slot_capacities.npz]

Prints the edges it could not reach and stores their names in `unreached`; only contacts_at, contacts_past and candidates_past may be missing."""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EDGES = ("limits_at", "limits_past", "frames_at", "frames_past", "contacts_at", "contacts_past", "candidates_16", "candidates_17", "candidates_20plus",
         "candidates_at", "candidates_past")
MAY_MISS = ("contacts_at", "contacts_past", "candidates_past")
N_LIGHT = 6
COUNTS = ("limits", "candidates", "contacts", "frames", "rows")
PEAKS = ("limits", "contacts", "frames", "rows")


def calm(c):
    """two away from the trip edge, and inside the candidate capacity"""
    return c["candidates"] <= 14 or 19 <= c["candidates"] <= 30


def inside(c, caps, skip=()):
    return all(c[k] <= caps[k] for k in c if k in caps and k not in skip)


class Search(object):
    def __init__(self):
        from oracle import oracle as O
        from tests import helpers as H
        from tests import rows_numpy as RW
        self.RW, self.cm = RW, H.compiled_model()
        self.om = H.oracle_model()
        self.probe = O.Data(self.om)
        self.found = {}
        self.light = []
        self.act_rng = np.random.RandomState(4242)

    def want(self):
        return [e for e in EDGES + ("norow",) if e not in self.found] + (["light"] if len(self.light) < N_LIGHT else [])

    def classify(self, c):
        """the entries the counts AT the state allow (the step's maxima are checked by offer)"""
        RW = self.RW
        caps = RW.CAPS
        names = []
        for k, edge in (("limits", "limits"), ("frames", "frames"), ("contacts", "contacts")):
            if c[k] == caps[k] and inside(c, caps) and calm(c):
                names.append(edge + "_at")
            if c[k] == caps[k] + 1 and inside(c, caps, skip=(k,)) and calm(c):
                names.append(edge + "_past")
        if inside(c, caps):
            if c["candidates"] == RW.TRIP:
                names.append("candidates_16")
            if c["candidates"] == RW.TRIP + 1 and c["late_contacts"] >= 1:
                names.append("candidates_17")
            if 20 <= c["candidates"] <= 30 and c["late_contacts"] >= 1:
                names.append("candidates_20plus")
            if c["candidates"] == caps["candidates"] and c["late_contacts"] >= 1:
                names.append("candidates_at")
            if c["rows"] == 0 and calm(c):
                names.append("norow")
            if 1 <= c["rows"] <= 11 and c["candidates"] < 8:
                names.append("light")
        if c["candidates"] == caps["candidates"] + 1 and inside(c, caps, skip=("candidates",)):
            names.append("candidates_past")
        return names

    def offer(self, frame, q, v, ws):
        """keeps the state for the first entry it fits and that is still open"""
        RW = self.RW
        c = RW.counts_at(self.cm, self.probe, q, v, ws)
        names = [n for n in self.classify(c) if (n == "light" and len(self.light) < N_LIGHT) or (n != "light" and n not in self.found)]
        if not names:
            return
        for _try in range(8):                                         # (a step's own action decides its later evaluations: up to eight are drawn)
            act = self.act_rng.randn(28) * 0.9
            self.probe.reset(); self.probe.set("qacc_warmstart", ws); self.probe.set_state(q, v)
            _o, _d, pk = RW.step_maxima(self.probe, act)
            entry = dict(frame=int(frame), qpos=np.array(q), qvel=np.array(v), ws=np.array(ws), action=act, counts=[c[k] for k in COUNTS], peaks=[pk[k] for k in PEAKS],
                         late=c["late_contacts"])
            for n in names:
                if not n.endswith("_past"):
                    own = n.split("_")[0]
                    if not inside(pk, RW.CAPS) or (n.endswith("_at") and own in pk and pk[own] != RW.CAPS[own]):
                        continue
                if n == "light":
                    self.light.append(entry)
                else:
                    self.found[n] = entry
                return


def limit_pose(cm, k):
    q = cm.qpos0.copy(); q[2] = 3.0
    hinges = [j for j in range(1, cm.njnt) if cm.jnt_limited[j]]
    for i, j in enumerate(hinges[:k]):
        q[cm.jnt_qposadr[j]] = cm.jnt_range[j][0] - 0.02 if i % 2 == 0 else cm.jnt_range[j][1] + 0.02
    return q


def rollouts(S, starts, steps):
    from oracle import oracle as O
    from deepmimic_mujoco_amd.mocap import ALL_CLIPS
    from tests import helpers as H
    od = O.Data(S.om)
    for s in range(starts):
        for ci, clip in enumerate(ALL_CLIPS):
            mc = H.mocap(clip)
            rng = np.random.RandomState(1000 * s + ci)
            f = int(rng.randint(0, mc.data_config.shape[0]))
            od.reset(); od.set_state(mc.data_config[f], mc.data_vel[f])
            for _t in range(steps):
                S.offer(f if clip == "walk" else 0, od.get("qpos").copy(), od.get("qvel").copy(), od.get("qacc_warmstart").copy())
                od.env_step(rng.randn(28) * 0.9)             # (on past a fall: a lying humanoid is where the contacts are)
            if not [w for w in S.want() if w not in MAY_MISS and w not in ("candidates_at",)]:
                return


def lying_poses(S, per=40):
    from deepmimic_mujoco_amd.mocap import ALL_CLIPS
    from tests import helpers as H
    for ci, clip in enumerate(ALL_CLIPS):
        _idx, q, v, ws, _ctrl = H.varied_states(per, seed=ci, clip=clip)
        rng = np.random.RandomState(77 + ci)
        for e in range(0, per, 5):
            q[e, 2] = 0.05 + 0.3 * rng.rand(); v[e] *= 0.3
        for e in range(per):
            q[e, 3:7] /= np.linalg.norm(q[e, 3:7])
            S.offer(0, q[e], v[e], ws[e])


def curled_poses(S, iters=6000):
    """a pose in the air climbed towards many broad-phase candidates: three joints moved at a time inside their ranges, a move kept when the candidate count
    does not fall while the contact pairs stay within 8 (and the contacts within 13)"""
    cm, RW = S.cm, S.RW
    lo = np.full(35, -3.0); hi = np.full(35, 3.0)
    for j in range(1, cm.njnt):
        if cm.jnt_limited[j]:
            lo[cm.jnt_qposadr[j]], hi[cm.jnt_qposadr[j]] = cm.jnt_range[j][0] + 1e-3, cm.jnt_range[j][1] - 1e-3
    rng = np.random.RandomState(5)
    q = cm.qpos0.copy(); q[2] = 3.0
    v = np.zeros(34)
    best = len(RW.candidate_pairs(cm, q))
    for _it in range(iters):
        if "candidates_at" in S.found and "candidates_past" in S.found:
            return
        q2 = q.copy(); k = rng.randint(7, 35, size=3); q2[k] += rng.randn(3) * 0.3
        q2[7:] = np.clip(q2[7:], lo[7:], hi[7:])
        n = len(RW.candidate_pairs(cm, q2))
        if n < best or n > RW.CAPS["candidates"] + 1:
            continue
        c = RW.counts_at(cm, S.probe, q2, v)
        if c["frames"] > RW.CAPS["frames"] or c["contacts"] > RW.CAPS["contacts"]:
            continue
        best, q = n, q2
        if n >= RW.CAPS["candidates"]:
            S.offer(0, q, v, np.zeros(34))


def write_npz(path, arrays):
    """an uncompressed .npz whose bytes depend on the arrays alone (numpy's own writer stamps every member with the time of day)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "slot_capacities.npz"))
    a = ap.parse_args()
    S = Search()
    for k in (16, 17):
        S.offer(0, limit_pose(S.cm, k), np.zeros(34), np.zeros(34))
    rollouts(S, starts=8, steps=200)
    lying_poses(S)
    curled_poses(S)
    unreached = [e for e in EDGES if e not in S.found]
    print("unreached:", unreached)
    bad = [e for e in unreached if e not in MAY_MISS]
    if bad or "norow" not in S.found or len(S.light) < N_LIGHT:
        print("the search did not reach %s (no-row state: %s, light states: %d of %d)" % (bad, "norow" in S.found, len(S.light), N_LIGHT))
        return 1
    names = [e for e in EDGES if e in S.found] + ["norow"] + ["light_%d" % i for i in range(N_LIGHT)]
    ent = [S.found[n] if n in S.found else S.light[int(n.split("_")[1])] for n in names]
    for n, e in zip(names, ent):
        print("%-18s %s at the state %s; largest of the step %s; contacts past candidate 15: %d" % (n, "/".join(COUNTS), e["counts"], e["peaks"], e["late"]))
    write_npz(a.out, dict(name=np.array(names), unreached=np.array(unreached, dtype="U32"), frame=np.array([e["frame"] for e in ent], dtype=np.int32),
                          qpos=np.array([e["qpos"] for e in ent]), qvel=np.array([e["qvel"] for e in ent]), qacc_warmstart=np.array([e["ws"] for e in ent]),
                          action=np.array([e["action"] for e in ent]), counts=np.array([e["counts"] for e in ent], dtype=np.int32),
                          peaks=np.array([e["peaks"] for e in ent], dtype=np.int32), late_contacts=np.array([e["late"] for e in ent], dtype=np.int32),
                          count_names=np.array(COUNTS), peak_names=np.array(PEAKS)))
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
