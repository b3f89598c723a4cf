#!/usr/bin/env python3
"""Record tests/golden/slot_variant_boundaries.npz: packed-step results of the wave testbench (tests/emu) at the row counts where
slot_forward changes its constraint-stage code (slot_kernel.h: one row set up to 16 rows, two up to 32, the partial third set beyond) and one row
short of them.

States come from oracle rollouts of `walk` under N(0, 0.9^2) actions; one state per boundary row count (14, 15, 16, 17, 30, 31, 32) leads a
wave, next to a partner without rows, a light partner and a second boundary state.  The recorded arrays are what the testbench of the
commit this script is run on computes — run it on the commit whose arithmetic is the reference, then commit the file; tests/
test_slot_variant_boundaries.py requires every later commit to reproduce them bit for bit.

    python3 tools/make_slot_variant_golden.py [--seed 1] [--out tests/golden/slot_variant_boundaries.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUNDARIES = (14, 15, 16, 17, 30, 31, 32)
T = 2


def collect(seed, starts=64, steps=150):
    """{row count: (frame, qpos, qvel, qacc_warmstart)} — the first state met with each row count, in rollout order"""
    from oracle import oracle as O
    from tests import helpers as H
    mc = H.mocap()
    om = H.oracle_model()
    rng = np.random.RandomState(seed)
    found = {}
    light = []
    od = O.Data(om); probe = O.Data(om)
    for _ in range(starts):
        f = int(rng.randint(0, mc.data_config.shape[0]))
        od.reset(); od.set_state(mc.data_config[f], mc.data_vel[f])
        for t in range(steps):
            st = (f, od.get("qpos").copy(), od.get("qvel").copy(), od.get("qacc_warmstart").copy())
            probe.reset(); probe.set_state(st[1], st[2])          # the row count AT the state (the rollout's own is the step's last evaluation's)
            ne = int(probe.get("nefc")[0])
            if ne not in found:
                found[ne] = st
            if 0 < ne < 12 and len(light) < 8:
                light.append(st)
            od.env_step(rng.randn(28) * 0.9)          # (on past a fall: a lying humanoid is where the high row counts are)
        if all(b in found for b in BOUNDARIES + (0,)) and len(light) >= 8:
            break
    return found, light


def arrange(found, light):
    """eight waves: seven led by a boundary state, the last one partly filled (two environments)"""
    envs = []
    for i, b in enumerate(BOUNDARIES):
        other = BOUNDARIES[(i + 3) % len(BOUNDARIES)]
        other = other if other <= b else BOUNDARIES[max(0, i - 1)]
        envs += [found[b], found[0], light[i % len(light)], found[other]]
    envs += [found[0], found[31]]
    idx = np.asarray([e[0] for e in envs], dtype=np.int32)
    q = np.asarray([e[1] for e in envs]); v = np.asarray([e[2] for e in envs]); ws = np.asarray([e[3] for e in envs])
    return idx, q, v, ws


def run(idx, q, v, ws, acts, mode, horizon):
    from deepmimic_mujoco_amd import _abi as A
    from tests import helpers as H
    from tests.emu.emu import EmuBatch
    mc = H.mocap()
    n = len(idx)
    b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, n, 0)
    b.set_option(A.OPT_PACKED, mode)
    b.set(A.F_QACC_WARMSTART, ws); b.set(A.F_TIME, np.zeros(n))
    b.set_state(q, v, frame_idx=idx)
    out = {"nefc0": b.get(A.F_NEFC).copy()}
    steps = acts.shape[0]
    if horizon:
        obs, rew, done = b.rollout(acts)
    else:
        obs = np.zeros((steps, n, 56)); rew = np.zeros((steps, n)); done = np.zeros((steps, n), dtype=np.uint8)
        qacc = np.zeros((steps, n, 34)); it = np.zeros((steps, n), dtype=np.int32); ne = np.zeros((steps, n), dtype=np.int32)
        for t in range(steps):
            b.step(acts[t], 1, out=(obs[t], rew[t], done[t]))
            qacc[t] = b.get(A.F_QACC_WARMSTART); it[t] = b.get(A.F_SOLVER_ITER); ne[t] = b.get(A.F_NEFC)
        out.update(qacc_steps=qacc, solver_iter_steps=it, nefc_steps=ne)
    out.update(obs=obs, reward=rew, done=done, qpos=b.get(A.F_QPOS), qvel=b.get(A.F_QVEL), qacc=b.get(A.F_QACC_WARMSTART),
               solver_iter=b.get(A.F_SOLVER_ITER), nefc=b.get(A.F_NEFC), redo=np.asarray(b.redo_total()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "slot_variant_boundaries.npz"))
    ap.add_argument("--search", action="store_true", help="only report which row counts the seed's rollouts reach")
    a = ap.parse_args()
    found, light = collect(a.seed)
    missing = [b for b in BOUNDARIES + (0,) if b not in found]
    print("seed %d: row counts met %s; missing %s; light %d" % (a.seed, sorted(found), missing, len(light)))
    if missing or len(light) < 8:
        return 1
    if a.search:
        return 0
    idx, q, v, ws = arrange(found, light)
    acts = np.random.RandomState(a.seed + 1000).randn(T, len(idx), 28) * 0.9
    # the reference: per-step launches with the three-set code compiled in (up to 40 rows stay on the packed path); the horizon form must give the same bits.
    # The lean per-step launches hand an environment that passes 32 rows inside a step to the one-env code: recorded beside it ("lean_").
    ref = run(idx, q, v, ws, acts, 2, False)
    hor = run(idx, q, v, ws, acts, 1, True)
    for k in ("obs", "reward", "done", "qpos", "qvel", "qacc", "solver_iter", "nefc", "redo", "nefc0"):
        assert np.array_equal(ref[k], hor[k]), "the per-step and the horizon form disagree on %s" % k
    lean = run(idx, q, v, ws, acts, 1, False)
    print("nefc at the states:", ref["nefc0"].tolist())
    print("nefc after each step:", ref["nefc_steps"].tolist())
    print("re-stepped by the one-env code: %d (three-set launches), %d (lean launches)" % (int(ref["redo"]), int(lean["redo"])))
    keys = ("obs", "reward", "done", "qpos", "qvel", "qacc", "solver_iter", "nefc", "qacc_steps", "solver_iter_steps", "nefc_steps", "redo")
    np.savez_compressed(a.out, seed=np.asarray(a.seed), frame=idx, qpos0=q, qvel0=v, qacc_warmstart0=ws, actions=acts, nefc0=ref["nefc0"],
                        **{k: ref[k] for k in keys}, **{"lean_" + k: lean[k] for k in keys})
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
