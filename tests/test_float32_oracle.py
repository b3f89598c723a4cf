"""The float32 build of the CPU oracle (liboracle32.so) and what tests/float32_cases.py derives from the two builds: the yardstick of
tests/test_gpu_float32.py, checked here without a GPU so that a regression of the float32 oracle cannot silently widen the GPU bars."""
import numpy as np

from tests import float32_cases as F
from tests import helpers as H


def test_float32_oracle_speaks_its_own_type_behind_a_float64_boundary():
    """Same source, one typedef: the float32 library's arrays are floats (every value it returns is a float32 number), callers pass and receive
    float64 arrays, and the default library is the float64 one."""
    from oracle import oracle as O
    assert O.lib().dmo_sizeof_real() == 8 and O.lib(32).dmo_sizeof_real() == 4 and O.lib(64) is O.lib()
    m64, m32 = O.Model(), O.Model(dtype=32)
    assert (m32.nq, m32.nv, m32.nu, m32.nbody) == (m64.nq, m64.nv, m64.nu, m64.nbody) and m32.dtype == 32 and m64.dtype == 64
    c = F.inputs()
    for m in (m64, m32):
        d = O.Data(m)
        d.set("qacc_warmstart", c["ws"][3]); d.set("ctrl", c["ctrl"][3]); d.set_state(c["q"][3], c["v"][3])
        q = d.get("qpos")
        assert q.dtype == np.float64 and np.array_equal(q, c["q"][3])                   # float32-rounded inputs survive either boundary exactly
        acc = d.get("qacc")
        assert np.array_equal(acc, F.f64r(acc)) == (m.dtype == 32)                       # 34 float64 results are not all float32 numbers
    s32 = O.humanoid_spec(32)
    assert isinstance(s32, O.Spec32) and abs(s32.timestep - 0.0166) < 1e-8 and s32.timestep != 0.0166
    assert O.Model(s32).dtype == 32


def test_float32_oracle_reproduces_the_reference_discrete_outcomes():
    """On every selected env and step the float32 oracle's nefc, ncon, contact list, done, frame index and cycle are the float64 oracle's; taken
    alone it disagrees on no more envs than the selection may drop."""
    R = F.reference()
    ref, o32, sel = R["ref"], R["o32"], R["selected"]
    for k in F.DISCRETE:
        same = (ref[k] == o32[k]).reshape(F.T + 1, F.N, -1).all(axis=2)
        assert same[sel].all(), k
        assert (~same).any(axis=0).mean() <= F.MAX_UNSELECTED, k
    it = (ref["solver_iter"] == o32["solver_iter"]).sum(axis=1)
    print("PGS sweep counts equal on %s of %d envs (initial evaluation, steps 1..3); stage evaluation: %d" %
          (it.tolist(), F.N, int((R["stage_iter"] == R["stage32_iter"]).sum())))


def test_selection_keeps_all_but_two_per_cent_and_the_sets_cover_every_row_class():
    R = F.reference()
    sel = R["selected"]
    sets = F.case_sets()
    for name, ids in sets.items():
        out = 1.0 - sel[:, ids].mean(axis=1)
        print("set %s: %d envs, unselected per step %s" % (name, len(ids), (~sel[:, ids]).sum(axis=1).tolist()))
        assert (out <= F.MAX_UNSELECTED).all(), (name, out)
    assert sel[0].all() and sel[1].all(), "every env of A is selected through the first step"
    assert [len(sets[k]) for k in ("n1", "n4", "n5", "n13")] == [1, 4, 5, 13]
    cls = F.row_class(R["rows_max"])
    for name, ids in sets.items():
        assert (cls[ids] == 3).any() and (name == "n1" or (cls[ids] <= 2).any()), "a 33 .. 40-row env beside lighter ones in %s" % name
    counts = np.bincount(cls, minlength=6)
    print("envs by largest row count (0, 1-16, 17-32, 33-40, 41-48, 49-63):", counts.tolist())
    assert (counts >= 4).all(), counts
    assert R["rows_max"].max() <= F.MAX_EFC
    done = R["ref"]["done"].any(axis=0)
    assert 0.1 < done.mean() < 0.9 and np.array_equal(R["ref"]["done"], R["ref"]["done_alive"])       # a looping clip: the height test alone ends an episode


def test_live_envelope_stays_within_the_recorded_one():
    """median and max of rel_err(oracle32, oracle64) per quantity, step and case set <= 1.5 x RECORDED (float32_cases.py); the obs maxima stay
    below 2e-5 (4 x the 4.3e-6 a float evaluation of the step measures on set A)."""
    assert sorted(F.RECORDED) == sorted(F.case_sets())
    for name in F.case_sets():
        env, rec = F.envelope(name), F.RECORDED[name]
        assert sorted(env) == sorted(rec) == sorted(F.ROLLOUT_Q + F.STAGE_Q)
        for k in F.ROLLOUT_Q + F.STAGE_Q:
            live = env[k] if k in F.ROLLOUT_Q else [env[k]]
            want = rec[k] if k in F.ROLLOUT_Q else [rec[k]]
            assert len(live) == len(want) == (F.T if k in F.ROLLOUT_Q else 1)
            for t, ((med, mx), (rmed, rmx)) in enumerate(zip(live, want)):
                assert med <= 1.5 * rmed and mx <= 1.5 * rmx, "%s %s step %d: live %.3e / %.3e, recorded %.3e / %.3e" % (name, k, t + 1, med, mx, rmed, rmx)
                assert rmed > 0 and rmx >= rmed                     # (a zero bar would ask the kernels for the reference's bits)
    for t, (med, mx) in enumerate(F.envelope("A")["obs"]):
        print("set A obs after step %d: median %.3e max %.3e" % (t + 1, med, mx))
        assert mx < 2e-5


def test_bars_are_the_margin_times_the_envelope():
    a = F.envelope("A")
    assert F.bars("A", "obs", 0) == (F.MARGIN * a["obs"][0][0], F.MARGIN * a["obs"][0][1])
    assert F.bars("A", "efc_force") == (F.MARGIN * a["efc_force"][0], F.MARGIN * a["efc_force"][1])
    assert F.bars("n4", "qvel", 2) == (None, F.MARGIN * a["qvel"][2][1])                    # a small set: A's max bar, no median bar
    assert F.bars("n13", "qvel", 2) == (F.MARGIN * F.envelope("n13")["qvel"][2][0], F.MARGIN * a["qvel"][2][1])
    assert F.MARGIN == 4.0 and F.MAX_UNSELECTED == 0.02 and F.N_DRAWS == 6 and F.REL_PERTURB == 1e-5
