"""Action modes 1..4 crossed with reward modes 2 ("v2-pose") and 4 ("v1-quat") on the wave testbench: the pairs whose frame rule and control
cost nothing else covers.  The kernel source (csrc/env_step.h, csrc/slot_step.h) runs lane for lane on CPU fibres against the float64 rows of
tests/action_reward_cases.py; tests/test_gpu_action_reward.py runs the same cases, and the remaining reward modes, on the device.

In reward modes 2 and 4 DM_F_FRAME_IDX counts the episode's steps and the drawn frame sits in DM_F_FRAME_INIT; the front ends of action modes 1, 2
and 4 must track (cursor + init) % F and (cursor // upd + init) % F, the frames those rewards count from.  Before env_step.h step_start_frame
they indexed the mocap tables with the cursor itself.  Run against those headers, 19 of these tests fail, every one with action modes 1, 2 and 4; worst
relative error (helpers.rel_err) of DM_F_CTRL, one env per wave / four per wave:
    action 1: reward 2  3.4 / 3.4     reward 4  3.9 / 3.5     reward 4, two substeps  0.80
    action 2: reward 2  7.6e+174 (memory past the tables) / 6.3     reward 4  6.6 / 3.0     reward 4, two substeps  5.4
    action 4: reward 2  2.1 / 1.5     reward 4  2.7 / 1.2     reward 4, two substeps  1.7
with obs off by 1.2 .. 2.8 and the reward by 0.2 .. 49 (inf where the read left the tables).  Action mode 3 reads no frame: its pairs pass before
and after and pin the control cost of reward modes 2 and 4 (the last substep's unclamped ctrl).

Bars: the testbench's parity bar is 1e-9.  Measured worst relative errors over the file: DM_F_CTRL 1.0e-14, obs 1.3e-14, reward 4.8e-15, final
qpos 2.8e-15, qacc_warmstart 7.5e-14; the tests hold them to 1e-12 (warm start 1e-11), as the other testbench tests tighten theirs.  4 envs x 4
steps per run; the file steps about 380 env-steps (35 s)."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from tests import action_reward_cases as AR
from tests import helpers as H
from tests.emu.emu import EmuBatch

TOL, WS_TOL = 1e-12, 1e-11
_PACKED_RUNS = {}


def _make(case, packed):
    mc = H.mocap()
    imit = AR.imit_inputs() if case["reward_mode"] >= 3 else None
    b = EmuBatch(H.compiled_model(), mc.data_config, mc.data_vel, case["n"], 0, imitation=imit, mocap_dt=float(mc.dt))
    b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_ACTION_MODE, case["action_mode"]); b.set_option(A.OPT_REWARD_MODE, case["reward_mode"])
    return b


def test_cases_contain_the_three_cursor_situations():
    """What the cases are made of, from the case data alone: in reward modes 2 and 4 a run of T = 4 steps has an env whose frame wraps modulo F
    while its cursor is far below F, one whose cursor itself passes F, and one far from either; mode 4's update interval is 2 with one substep
    and 1 with two on `walk`."""
    F = H.mocap().data_config.shape[0]
    assert (AR.upd_of(4, 1), AR.upd_of(4, 2)) == (2, 1)
    for rm, nsub in ((2, 1), (4, 1), (4, 2)):
        for n in (4, 13):
            case = AR.make_case(1, rm, nsub, n=n)
            cur, fr = AR.situations(case)
            wraps = [e for e in range(n) if cur[:, e].max() < F - 8 and np.any(np.diff(fr[:, e]) < 0)]
            passes = [e for e in range(n) if cur[0, e] < F <= cur[-1, e]]
            far = [e for e in range(n) if cur[:, e].max() < F - 8 and fr[:, e].max() < F - 4 and np.all(np.diff(fr[:, e]) >= 0)]
            assert wraps and passes and far, (rm, nsub, n, cur, fr)
            assert np.any(cur != fr) and fr.min() >= 0 and fr.max() < F


@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("rm", [2, 4])
@pytest.mark.parametrize("am", [1, 2, 3, 4])
def test_pairs_match_the_reference_on_the_testbench(am, rm, packed):
    """One env per wave (env_step.h) and four per wave (slot_step.h): DM_F_CTRL and both cursors after every step, obs / reward / done every
    step, the final qpos / qacc_warmstart / time, every env of the batch."""
    case = AR.make_case(am, rm)
    b = _make(case, packed)
    got = AR.run_steps(b, case)
    if packed:
        _PACKED_RUNS[(am, rm)] = got
    worst = AR.check(case, AR.expected(case), got, tol=TOL, ws_tol=WS_TOL)
    print("testbench action %d reward %d packed %d: worst rel err %s" % (am, rm, packed, worst))


@pytest.mark.parametrize("am,packed", [(1, 0), (2, 1), (3, 0), (4, 1)])
def test_v1_reward_with_two_substeps_on_the_testbench(am, packed):
    """Reward mode 4 with two substeps per env step: the update interval is 1 instead of 2, so the front ends' frame is cursor + init; in action
    modes 3 and 4 the control cost is the SECOND substep's ctrl."""
    case = AR.make_case(am, 4, nsub=2)
    assert AR.upd_of(4, 2) != AR.upd_of(4, 1)
    exp = AR.expected(case)
    worst = AR.check(case, exp, AR.run_steps(_make(case, packed), case), tol=TOL, ws_tol=WS_TOL)
    if am >= 3:
        one = AR.expected(AR.make_case(am, 4, nsub=1))
        assert np.abs(exp["ctrl"][0] - one["ctrl"][0]).max() > 1e-3, "the second substep's ctrl must differ from the first's for the cost to tell them apart"
    print("testbench action %d reward 4, two substeps, packed %d: worst rel err %s" % (am, packed, worst))


@pytest.mark.parametrize("rm", [2, 4])
@pytest.mark.parametrize("am", [1, 2])
def test_horizon_form_equals_packed_steps_bit_for_bit(am, rm):
    """slot_rollout (the horizon launch's body) steps through the same front end: rows, cursors, final state and the last ctrl are the packed
    per-step run's, bit for bit."""
    case = AR.make_case(am, rm)
    ref = _PACKED_RUNS.get((am, rm)) or AR.run_steps(_make(case, 1), case)
    got = AR.run_steps(_make(case, 1), case, horizon=True)
    AR.same_bits(got, ref)
    AR.check(case, AR.expected(case), got, tol=TOL, ws_tol=WS_TOL)


def test_spd_restatement_of_the_v1_epilogue_is_the_oracles():
    """tests/spd_numpy.py restates dmo_env_step_v1's epilogue (a zero-substep call cannot be asked of it): with the oracle's own ctrl held
    through the substeps the two must agree to rounding — checked by replaying env_step_v1's rows through the restated epilogue."""
    from oracle import oracle as O
    from tests import spd_numpy as S
    mc, om = H.mocap(), H.oracle_model()
    tab, par = AR.imit_inputs()
    F = len(tab)
    idx, q, v, _w, _c = H.varied_states(3, seed=9)
    rng = np.random.RandomState(4)
    for nsub in (1, 2):
        upd = AR.upd_of(4, nsub)
        for e in range(3):
            od = O.Data(om); od.reset(); od.set_state(q[e], v[e])
            cur = F - 2
            for t in range(4):
                a = rng.randn(28) * 0.3
                o, r, d, nxt = O.env_step_v1(om, od, a, nsub, tab, par, float(mc.dt), cur, int(idx[e]))
                want = 0.0
                if nxt % upd == 0:
                    k = (nxt // upd + int(idx[e])) % F
                    want = O.v1_reward(om, O.imitation_features(om, od.get("qpos", 40), od.get("qvel", 40), par), tab[k], tab[min(k + 1, F - 1)], par)[0]
                assert abs(want - 0.1 * np.square(a).sum() - r) < 1e-14 and nxt == cur + 1
                assert S.start_frame(4, nxt, int(idx[e]), F, upd) == (nxt // upd + int(idx[e])) % F
                cur = nxt
