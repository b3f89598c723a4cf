"""Multi-clip batches without a GPU: the host-side ClipSet (concatenation, records, cdf, validation), the C entry point's argument checks, and
the clip instantiations of the step and reset routines on the wave testbench (tests/emu_clips) — against the oracle env by env, against
single-clip twins bit for bit, and the episode-mode draw against its host mirror — in both lane layouts.  tests/clips_cases.py has the
test set and the references; tests/test_gpu_clips_multi.py runs them on the device."""
import ctypes as C

import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.clips import ClipSet, clip_cdf, draw_clip
from tests import clips_cases as CC
from tests import helpers as H


# ---- ClipSet ---------------------------------------------------------------------------------------------------------------------------
def test_clip_set_concatenation_records_and_cdf():
    cs = CC.clip_set(weights=(1, 0, 3))
    mcs = [H.mocap(c) for c in CC.NAMES]
    F = [m.data_config.shape[0] for m in mcs]
    assert F == [39, 78, 47] and list(cs.n_frames) == F and list(cs.row0) == [0, 39, 117]
    assert cs.data_config.shape == (sum(F), 35) and cs.data_vel.shape == (sum(F), 34) and cs.imit_table.shape == (sum(F), 112)
    for k, m in enumerate(mcs):
        rows = slice(int(cs.row0[k]), int(cs.row0[k]) + F[k])
        assert np.array_equal(cs.data_config[rows], m.data_config) and np.array_equal(cs.data_vel[rows], m.data_vel)
        assert np.array_equal(cs.imit_table[rows], cs.imitation[k][0])
    rec = cs.records()
    assert [r["dt"] for r in rec] == [float(m.dt) for m in mcs] and rec[0]["dt"] != rec[1]["dt"]
    assert [r["loop"] for r in rec] == [1.0, 1.0, 0.0]                       # kick is "Loop: none"
    for k, r in enumerate(rec):
        p = cs.imitation[k][1]
        assert (r["shift_x"], r["shift_y"], r["loop"]) == (p[13], p[14], p[15])
    # the cdf: float64 running sum over the total, a zero-weight clip repeats its predecessor's entry and is never drawn, the last entry is 1.0 exactly
    assert list(cs.cdf) == [0.25, 0.25, 1.0]
    assert [draw_clip(cs.cdf, u) for u in (0.0, 0.2499999, 0.25, 0.9999999)] == [0, 0, 2, 2]
    third = clip_cdf([1, 1, 1])
    assert third[-1] == 1.0 and third[0] == 1.0 / 3.0 and third[1] == (1.0 + 1.0) / 3.0
    assert clip_cdf([0.1] * 7)[-1] == 1.0
    assert list(CC.clip_set(weights=(0, 1, 0)).cdf) == [0.0, 1.0, 1.0]
    assert list(cs.default_assignment(5, env_offset=2)) == [2, 0, 1, 2, 0]


def test_clip_set_validation():
    with pytest.raises(ValueError):
        ClipSet([])
    with pytest.raises(ValueError):
        ClipSet(["walk"] * (A.MAX_CLIPS + 1))
    for w in ((1, -1, 1), (0, 0, 0), (1, float("nan"), 1), (1, float("inf"), 1), (1, 1)):
        with pytest.raises(ValueError):
            ClipSet([H.mocap(c) for c in CC.NAMES], w)

    class Spec(object):            # a spec whose shared parameters differ from clip to clip
        def __init__(self):
            self.k = 0

        def table_for(self, m):
            p = np.zeros(32); p[0] = self.k; self.k += 1
            return np.zeros((m.data_config.shape[0], 112)), p
    with pytest.raises(ValueError):
        ClipSet([H.mocap("walk"), H.mocap("kick")], None, Spec())


def _c_mocap(L, m, imit=None):
    cfg = np.ascontiguousarray(m.data_config); vel = np.ascontiguousarray(m.data_vel)
    h = C.c_void_p()
    assert L.dm_mocap_create(cfg.ctypes.data_as(A._dp), vel.ctypes.data_as(A._dp), cfg.shape[0], float(m.dt), C.byref(h)) == 0
    if imit is not None:
        tab = np.ascontiguousarray(imit[0]); par = np.ascontiguousarray(imit[1])
        assert L.dm_mocap_set_imitation(h, tab.ctypes.data_as(A._dp), 112, par.ctypes.data_as(A._dp)) == 0
    return h


@pytest.mark.parametrize("dtype", [64, 32])
def test_mocap_create_set_validates_on_the_host(dtype):
    """dm_mocap_create_set touches no device: its argument rules hold in both libraries"""
    L = A.load(dtype)
    cs = CC.clip_set()
    hs = [_c_mocap(L, m, cs.imitation[k]) for k, m in enumerate(cs.mocaps)]
    arr = (C.c_void_p * 3)(*[h.value for h in hs])
    out = C.c_void_p()
    w = lambda *x: np.asarray(x, dtype=np.float64).ctypes.data_as(A._dp)
    assert L.dm_mocap_create_set(arr, 3, None, C.byref(out)) == 0 and out.value
    nested = (C.c_void_p * 2)(hs[0].value, out.value)
    out2 = C.c_void_p()
    assert L.dm_mocap_create_set(nested, 2, None, C.byref(out2)) == -1 and b"single clip" in L.dm_last_error()
    L.dm_mocap_destroy(out)
    assert L.dm_mocap_create_set(arr, 3, w(1, 2, 1), C.byref(out)) == 0
    L.dm_mocap_destroy(out)
    assert L.dm_mocap_create_set(arr, 0, None, C.byref(out)) == -1 and L.dm_mocap_create_set(arr, A.MAX_CLIPS + 1, None, C.byref(out)) == -1
    assert L.dm_mocap_create_set(None, 3, None, C.byref(out)) == -1 and L.dm_mocap_create_set(arr, 3, None, None) == -1
    for bad in ((1, -1, 1), (0, 0, 0), (1, float("nan"), 1), (1, float("inf"), 1)):
        assert L.dm_mocap_create_set(arr, 3, w(*bad), C.byref(out)) == -1 and b"weights" in L.dm_last_error()
    # either all clips carry an imitation table or none; the shared parameters must agree
    bare = _c_mocap(L, cs.mocaps[1])
    mixed = (C.c_void_p * 2)(hs[0].value, bare.value)
    assert L.dm_mocap_create_set(mixed, 2, None, C.byref(out)) == -1 and b"either every clip" in L.dm_last_error()
    par = np.array(cs.imitation[1][1]); par[3] += 0.5
    odd = _c_mocap(L, cs.mocaps[1], (cs.imitation[1][0], par))
    differ = (C.c_void_p * 2)(hs[0].value, odd.value)
    assert L.dm_mocap_create_set(differ, 2, None, C.byref(out)) == -1 and b"must be equal across the set" in L.dm_last_error()
    par = np.array(cs.imitation[1][1]); par[13] += 0.5; par[15] = 0      # 13..15 are per clip: accepted
    own = _c_mocap(L, cs.mocaps[1], (cs.imitation[1][0], par))
    assert L.dm_mocap_create_set((C.c_void_p * 2)(hs[0].value, own.value), 2, None, C.byref(out)) == 0
    L.dm_mocap_destroy(out)
    for h in hs + [bare, odd, own]:
        L.dm_mocap_destroy(h)
    hdr = open(H.GOLDEN + "/../../include/dmenv.h").read()
    assert "#define DM_OPT_CLIP_MODE %d" % A.OPT_CLIP_MODE in hdr and "DM_F_CLIP = %d" % A.F_CLIP in hdr and "#define DM_MAX_CLIPS %d" % A.MAX_CLIPS in hdr


def test_episode_mirror_draws_every_clip():
    """the seed of the episode-mode tests: with weights (1, 2, 1), 12 envs and 3 resets the host mirror draws every clip at least once"""
    cs = CC.clip_set(weights=(1, 2, 1))
    clip, _frame = CC.episode_mirror(cs, CC.EPISODE_SEED, 12, 3)
    assert set(clip.ravel().tolist()) == {0, 1, 2}
    assert [cs.episode_clip(CC.EPISODE_SEED, e, 0) for e in range(12)] == clip[0].tolist()


# ---- the clip instantiations on the wave testbench ---------------------------------------------------------------------------------------------
def _emu(cs, n, packed, reward_mode, action_mode=0, autoreset=0, seed=0, env_offset=0, clip_mode=0):
    from tests.emu_clips.emu_clips import EmuClipBatch
    b = EmuClipBatch(H.compiled_model(), cs, n)
    b.set_option(A.OPT_REWARD_MODE, reward_mode); b.set_option(A.OPT_ACTION_MODE, action_mode); b.set_option(A.OPT_AUTORESET, autoreset)
    b.set_option(A.OPT_SEED, seed); b.set_option(A.OPT_PACKED, packed); b.set_option(A.OPT_ENV_OFFSET, env_offset); b.set_option(A.OPT_CLIP_MODE, clip_mode)
    return b


def _emu_twin(cs, k, n, packed, reward_mode, autoreset, seed):
    from tests.emu.emu import EmuBatch
    m = cs.mocaps[k]
    b = EmuBatch(H.compiled_model(), m.data_config, m.data_vel, n, imitation=cs.imitation[k], mocap_dt=float(m.dt))
    b.set_option(A.OPT_REWARD_MODE, reward_mode); b.set_option(A.OPT_AUTORESET, autoreset); b.set_option(A.OPT_SEED, seed); b.set_option(A.OPT_PACKED, packed)
    return b


@pytest.mark.parametrize("packed", [0, 1])
@pytest.mark.parametrize("action_mode", [0, 1, 4])
@pytest.mark.parametrize("reward_mode", [1, 2, 3, 4])
def test_oracle_env_by_env_on_testbench(reward_mode, action_mode, packed):
    """each env of the mixed batch against an oracle Data stepped with its own clip's tables, parameters and dt: the device test's whole cross — N = 10,
    8 steps, reward modes 1..4 x action modes 0, 1, 4 x both layouts (about 7 s a case here)"""
    CC.check_oracle(_emu(CC.clip_set(), CC.N, packed, reward_mode, action_mode), reward_mode, action_mode)


def _twin_seed(T):
    """a seed whose RSI draw (helpers.device_rsi_frame: the mirror, not the code under test) puts a kick env's SECOND episode within reach of the clip's end:
    the env ends at step 3 from its start frame F - 3, is reset to the drawn frame f, and ends again by step T when f + (T - 3) >= F - 1"""
    F = 47
    for seed in range(1, 200):
        if any(H.device_rsi_frame(seed, e, 0, F) + (T - 3) >= F - 1 and H.device_rsi_frame(seed, e, 0, F) < F - 2 for e in (2, 5, 8)):
            return seed
    raise AssertionError("no seed")


TWIN_STEPS = 12      # the device test runs the issue's 48 steps; here a step of the four batches is 40 testbench env-steps (about 4 s), and 12 steps
                     # still hold a wrap with a counted cycle, a clip end with its auto-reset, and a drawn episode that itself reaches the clip's end


@pytest.mark.parametrize("autoreset", [1, 2], ids=["rsi", "init"])
@pytest.mark.parametrize("packed", [0, 1])
def test_twins_on_testbench(packed, autoreset):
    """env e of the multi-clip batch is env e of the single-clip batch of clip e % 3, bit for bit, N = 10, with both auto-reset modes ("init": mode 1 with
    `hard`, which draws the frame as well), through a wrap, a clip end, its auto-reset and a second clip end inside the drawn episode"""
    cs = CC.clip_set()
    n, seed = CC.N, _twin_seed(TWIN_STEPS)
    multi = _emu(cs, n, packed, 3, autoreset=autoreset, seed=seed)
    twins = [_emu_twin(cs, k, n, packed, 3, autoreset, seed) for k in range(3)]
    dones = CC.check_twins(multi, twins, TWIN_STEPS)
    assert dones[2, 2::3].all() and not dones[:3, 0::3].any()      # every kick env ended at its third step (and was reset); walk wrapped instead
    assert (dones[:, 2::3].sum(0) >= 2).any()                      # a drawn episode reached the clip's end again
    assert np.array_equal(multi.get(A.F_CLIP), np.arange(n) % 3)
    assert (multi.get(A.F_FRAME_INIT)[2::3] != CC.start(n)[1][2::3]).any()      # the reset drew the frame (both modes set the cursor)


def test_trainer_flags_for_a_list_of_motions():
    """--motion a,b,c, --clip-weights and --clip-mode of the three trainers (tools/_train_common.py): what reaches DPVecEnv, and the refused combinations"""
    import argparse
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
    import _train_common as common

    def parse(*argv):
        ap = argparse.ArgumentParser()
        common.add_env_args(ap, reward_help="r", autoreset_help="a", frame_skip_help="f")
        args = ap.parse_args(list(argv))
        common.check_env_args(ap, args)
        return common.env_kwargs(args)
    kw = parse()
    assert kw["motion"] == "walk" and kw["clip_weights"] is None and kw["clip_mode"] == "fixed"
    kw = parse("--motion", "walk,spinkick,kick", "--clip-weights", "1,2,1", "--clip-mode", "episode")
    assert kw["motion"] == ["walk", "spinkick", "kick"] and kw["clip_weights"] == [1.0, 2.0, 1.0] and kw["clip_mode"] == "episode"
    kw = parse("--motion", "walk,kick", "--max-episode-steps", "5", "--horizon-termination")      # passed through: the library issues step launches
    assert kw["motion"] == ["walk", "kick"] and kw["horizon_termination"] is True
    for bad in (("--clip-weights", "1,2"), ("--clip-mode", "episode"), ("--motion", "walk,kick", "--clip-weights", "1,2,3"),
                ("--motion", "walk,kick", "--clip-weights", "1,x")):
        with pytest.raises(SystemExit):
            parse(*bad)


def test_clip_write_holds_cursors_inside_the_new_clip_on_testbench():
    """the rule dm_batch_set(DM_F_CLIP) applies (mirrored by the testbench front end): a cursor naming a row beyond the new clip becomes its last frame, so the
    step that follows reads the clip's own rows — checked against the oracle stepped on kick's last frame"""
    from oracle import oracle as O
    cs = CC.clip_set()
    b = _emu(cs, 2, 0, 1)
    b.set(A.F_CLIP, np.array([1, 1], dtype=np.int32))
    m = cs.mocaps[1]
    fr = np.array([70, 10], dtype=np.int32)
    CC.prepare(b, fr, m.data_config[fr], m.data_vel[fr])
    b.set(A.F_CLIP, np.array([2, 1], dtype=np.int32))
    assert list(b.get(A.F_FRAME_IDX)) == [46, 10] and list(b.get(A.F_FRAME_INIT)) == [46, 10]
    a = np.zeros((2, 28))
    o, r, d = b.step(a)
    od = O.Data(H.oracle_model()); od.reset(); od.set_state(m.data_config[70], m.data_vel[70])
    oo, rr, dd, cur = od.env_step(a[0], 1, 1, cs.mocaps[2].data_config, 46, 46)
    assert H.rel_err(o[0], oo) < 1e-9 and abs(r[0] - rr) < 1e-9 and b.get(A.F_FRAME_IDX)[0] == cur == 0


@pytest.mark.parametrize("packed", [0, 1])
def test_episode_mode_on_testbench(packed):
    """dm_batch_reset and the in-kernel auto-reset draw the clip, then the frame over the drawn clip's length: the host mirror, reset by reset"""
    cs = CC.clip_set(weights=(1, 2, 1))
    n, seed = 12, CC.EPISODE_SEED
    b = _emu(cs, n, packed, 3, autoreset=1, seed=seed, clip_mode=1)
    clip, frame = CC.episode_mirror(cs, seed, n, 3)
    assert set(clip.ravel().tolist()) == {0, 1, 2}
    for r in range(3):
        b.reset(0, 1)
        assert np.array_equal(b.get(A.F_CLIP), clip[r]) and np.array_equal(b.get(A.F_FRAME_INIT), frame[r]) and np.array_equal(b.get(A.F_FRAME_IDX), frame[r])
        q = b.get(A.F_QPOS)
        for e in range(n):
            assert np.array_equal(q[e], cs.mocaps[clip[r, e]].data_config[frame[r, e]])
    # mode 1 without `hard` keeps clip and cursor; mode 2 likewise
    b.reset(1, 0); b.reset(2, 1)
    assert np.array_equal(b.get(A.F_CLIP), clip[2]) and np.array_equal(b.get(A.F_FRAME_INIT), frame[2])
    # the auto-reset inside the step: drop env 1 below the COM band, its episode (counter 5 by now) starts on the mirror's clip and frame
    ep = int(b.get(A.F_EPISODE)[1])
    q = b.get(A.F_QPOS); q[1, 2] = 0.3
    b.set_state(q, b.get(A.F_QVEL))
    _o, _r, d = b.step(np.zeros((n, 28)))
    c1, f1 = CC.episode_mirror(cs, seed, n, 1, episode0=ep)
    assert d[1] == 1 and b.get(A.F_CLIP)[1] == c1[0, 1] and b.get(A.F_FRAME_INIT)[1] == f1[0, 1] and b.get(A.F_EPISODE)[1] == ep + 1
    keep = d == 0
    assert np.array_equal(b.get(A.F_CLIP)[keep], clip[2][keep])
    # dm_batch_reset mode 1 with `hard` sets the cursor too, so it draws the clip as well (reset_commit's condition)
    eps = b.get(A.F_EPISODE).copy()
    b.reset(1, 1)
    for e in range(n):
        c, f = CC.episode_mirror(cs, seed, n, 1, episode0=int(eps[e]))
        assert b.get(A.F_CLIP)[e] == c[0, e] and b.get(A.F_FRAME_INIT)[e] == f[0, e]
    # weights (0, 1, 0) put every env on clip 1
    b2 = _emu(CC.clip_set(weights=(0, 1, 0)), 4, packed, 3, seed=seed, clip_mode=1)
    b2.reset(0, 1)
    assert (b2.get(A.F_CLIP) == 1).all()
