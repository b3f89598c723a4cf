"""Every select of a step call's part launch with a push schedule AND early termination on: the single-tier form (option 102 = 0), the profiled forms
(option 101) and DM_OPT_PIPELINE 2 against the plain form of their class, bit for bit.  The one-env kernels "perform identical arithmetic on the rows that
exist" (csrc/dmenv.hip) and profiles/host_split.md section 2 records one digest per class; here k_push precedes and k_terminate follows every form.

Setup: a walk batch (the multi-clip case: walk / spinkick / kick, clip mode "episode"), tests/push_cases.py's busy schedule, a limit of 5 steps per episode
with auto-reset 1, a fixed seed, 8 steps with device tensors (what DM_OPT_PIPELINE needs to pipeline).  Compared: observations, rewards, done, the state
fields of tests/test_gpu_push.py, DM_F_PUSH_STATE, DM_F_EPISODE_STEPS and DM_F_DONE_REASON.  Bar: bit for bit."""
import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch
from tests import clips_cases as CC
from tests import helpers as H
from tests import push_cases as PC
from tests.gpu_batch import STATE, assert_bits, horizon_rows, result, state_of

pytestmark = pytest.mark.gpu
STEPS, LIMIT = 8, 5
FIELDS = STATE + (A.F_PUSH_STATE, A.F_EPISODE_STEPS, A.F_DONE_REASON)
_PLAIN = {}


def configure(b, packed, options):
    b.set_option(A.OPT_SEED, PC.SEED); b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_AUTORESET, 1); b.set_option(A.OPT_MAX_EPISODE_STEPS, LIMIT)
    for opt, v in options:
        b.set_option(opt, v)
    b.set_push_schedule(PC.busy_schedule())
    b.reset(0, 1)


def run(b):
    """STEPS device-tensor steps -> the stacked outputs and the final fields"""
    n = b.n
    acts, *out = horizon_rows(STEPS, n, act=np.random.RandomState(4).randn(STEPS, n, A.NU) * 0.3)[:4]
    for t in range(STEPS):
        b.step(acts[t], 1, (out[0][t], out[1][t], out[2][t]))
    return result(b, out, FIELDS)


def walk(n, packed, options=()):
    mc = H.mocap()
    b = Batch(H.compiled_model(), mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt))
    configure(b, packed, options)
    res = run(b)
    b.close()
    return res


def plain(n, packed):
    """the class's plain form, computed once per (n, class) and shared (do not modify); asserts from the reference side that the limit ended episodes and
    that the schedule pushed"""
    if (n, packed) not in _PLAIN:
        res = walk(n, packed)
        assert res["rows2"].any(axis=0).all() and res[A.F_EPISODE].min() >= 1 + STEPS // LIMIT and res[A.F_EPISODE_STEPS].max() <= STEPS - LIMIT
        assert res[A.F_PUSH_STATE][:, 4].max() >= 1
        for x in res.values():
            x.setflags(write=False)
        _PLAIN[(n, packed)] = res
    return _PLAIN[(n, packed)]


@pytest.mark.parametrize("n,options", [(5, ((102, 0),)), (5, ((101, 1),)), (8, ((A.OPT_PIPELINE, 2),))], ids=["single-tier", "profiled", "pipeline-2"])
def test_one_env_selects_equal_the_two_tier_form(n, options):
    assert_bits(plain(n, 0), walk(n, 0, options), options)


@pytest.mark.parametrize("n,options", [(5, ((101, 1),)), (8, ((A.OPT_PIPELINE, 2),))], ids=["profiled", "pipeline-2"])
def test_packed_selects_equal_the_plain_packed_form(n, options):
    """5 envs: the second slot group is partial"""
    assert_bits(plain(n, 1), walk(n, 1, options), options)


def test_multi_clip_single_tier_equals_two_tier_and_profiling_stays_refused():
    cs = CC.clip_set()
    res = []
    for two_tier in (1, 0):
        b = Batch(H.compiled_model(), None, None, 5, device=0, clips=cs)
        configure(b, 0, ((A.OPT_REWARD_MODE, 3), (A.OPT_CLIP_MODE, A.CLIP_EPISODE), (102, two_tier)))
        res.append(run(b))
        res[-1][A.F_CLIP] = b.get(A.F_CLIP)
        if not two_tier:              # option 101 on a multi-clip batch: refused before anything is launched, and the batch steps on afterwards
            before = state_of(b, FIELDS)
            b.set_option(101, 1)
            with pytest.raises(A.DmenvError) as ei:
                b.step(np.zeros((5, A.NU)))
            assert "-4" in str(ei.value)
            assert_bits(before, state_of(b, FIELDS), "refused step")
            b.set_option(101, 0)
            b.step(np.zeros((5, A.NU)))
            assert b.get(A.F_TIME).tobytes() != before[A.F_TIME].tobytes()
        b.close()
    assert res[0]["rows2"].any() and res[0][A.F_PUSH_STATE][:, 4].max() >= 1
    assert_bits(res[0], res[1], "multi-clip single-tier")
