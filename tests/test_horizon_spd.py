"""Action modes 3 and 4 inside the horizon launch (DM_OPT_HORIZON_SPD; csrc/kernels_rollout_spd.hip, slot_step.h's SPD switch), without a GPU: the
option's id in the header, the Python mirror and both libraries, DPVecEnv's argument errors, the trainers' flag, and the wave-testbench twin — the
kernel source on CPU fibres under the sanitizers, slot_rollout with the controller inside against the packed step and the one-env re-steps as the
step launches run them, bit for bit.  tests/test_gpu_horizon_spd.py has the device."""
import os
import re
import subprocess
import time

import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import DPVecEnv
from deepmimic_mujoco_amd import termination as T
from tests import helpers as H
from tests import horizon_term_cases as HC
from tests.emu import hostprog as HP

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the id ---------------------------------------------------------------------------------------------------------------------------------
def test_header_and_python_mirror_agree():
    hdr = open(os.path.join(ROOT, "include", "dmenv.h")).read()
    assert int(re.search(r"^#define DM_OPT_HORIZON_SPD (\d+)", hdr, flags=re.M).group(1)) == A.OPT_HORIZON_SPD == 14
    assert int(re.search(r"#define DM_ABI_VERSION (\d+)", hdr).group(1)) == A.ABI_VERSION == 9      # one id added, no export, nothing moved
    ids = [int(m) for m in re.findall(r"^\s*DM_OPT_[A-Z_]+ = (\d+)", hdr, flags=re.M)]
    assert max(ids) == 12 and A.OPT_HORIZON_SPD not in ids and A.OPT_HORIZON_SPD != A.OPT_CLIP_MODE      # a #define beside DM_OPT_CLIP_MODE, not an enum entry
    # the paragraphs that said modes 3 and 4 never queue name the exception
    assert len(re.findall(r"unless\s+(?:\*\s+)?DM_OPT_HORIZON_SPD", hdr)) >= 3


@pytest.mark.parametrize("dtype", [64, 32])
def test_both_libraries_refuse_the_option_without_a_batch(dtype):
    """an option call is refused on the host where there is no batch (the values a batch accepts and refuses are tests/test_gpu_horizon_spd.py's)"""
    L = A.load(dtype)
    for v in (0, 1, 2, -1):
        assert L.dm_batch_set_option(None, A.OPT_HORIZON_SPD, v) == -1 and b"null" in L.dm_last_error()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------------
def test_vec_env_argument_errors_come_before_any_device_call(monkeypatch):
    from deepmimic_mujoco_amd import dp_env

    made = []

    def no_device(*a, **k):
        made.append(1)
        raise AssertionError("a batch was created")
    monkeypatch.setattr(dp_env, "Batch", no_device)
    for mode in ("raw", "p-control", "pd"):
        with pytest.raises(ValueError, match="spd-target"):
            DPVecEnv(8, horizon_spd=True, action_mode=mode)
    with pytest.raises(ValueError, match="deepmimic"):
        DPVecEnv(8, horizon_spd=True, action_mode="spd-mocap", obs_mode="deepmimic")
    # termination inside the horizon in an spd mode: only together with horizon_spd; the earlier error stays word for word
    for mode in ("spd-target", "spd-mocap"):
        with pytest.raises(ValueError, match="no horizon launch") as ei:
            DPVecEnv(8, horizon_termination=True, max_episode_steps=3, fall_contact_bodies="deepmimic", action_mode=mode)
        assert str(ei.value) == "horizon_termination=True: action_mode=%r runs on the per-step kernels, there is no horizon launch to terminate in" % (mode,)
    with pytest.raises(ValueError, match="fall_contact_bodies or max_episode_steps"):
        DPVecEnv(8, horizon_termination=True, horizon_spd=True, action_mode="spd-target")
    assert not made
    # valid combinations go on to the batch: alone, with termination, with a list of motions and with a push schedule (the library issues step launches there)
    for kw in (dict(), dict(horizon_termination=True, max_episode_steps=3), dict(motion=["walk", "kick"]),
               dict(perturb="bodies=deepmimic,force=50:100,duration=1:3,wait=5:9")):
        n0 = len(made)
        with pytest.raises(AssertionError, match="a batch was created"):
            DPVecEnv(8, horizon_spd=True, action_mode="spd-mocap", **kw)
        assert len(made) == n0 + 1


def test_train_tools_take_and_check_the_flag(capsys):
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import _train_common as common
    finally:
        sys.path.pop(0)
    ap = argparse.ArgumentParser()
    common.add_env_args(ap, reward_help="r")
    ok = ap.parse_args(["--horizon-spd", "--action-mode", "spd-target"])
    common.check_env_args(ap, ok)
    assert common.env_kwargs(ok)["horizon_spd"] is True and common.env_kwargs(ap.parse_args([]))["horizon_spd"] is False
    both = ap.parse_args(["--horizon-spd", "--action-mode", "spd-mocap", "--horizon-termination", "--max-episode-steps", "600", "--fall-contact", "deepmimic"])
    common.check_env_args(ap, both)
    kw = common.env_kwargs(both)
    assert kw["horizon_spd"] is True and kw["horizon_termination"] is True
    common.check_env_args(ap, ap.parse_args(["--horizon-spd", "--action-mode", "spd-mocap", "--motion", "walk,kick"]))      # passed through
    for bad in (["--horizon-spd"], ["--horizon-spd", "--action-mode", "pd"], ["--horizon-spd", "--action-mode", "spd-target", "--obs-mode", "deepmimic"],
                ["--horizon-termination", "--max-episode-steps", "5", "--action-mode", "spd-target"]):
        with pytest.raises(SystemExit):
            common.check_env_args(ap, ap.parse_args(bad))
    assert "--horizon-spd" in capsys.readouterr().err


# ---- the twin on the wave testbench -----------------------------------------------------------------------------------------------------------
MANY_ENV = 4          # the env that starts in a many-row state: the first slot of the second wave


def test_horizon_with_the_controller_equals_step_launches_on_the_wave_testbench(tmp_path):
    """6 envs (one full wave and one with two spare slots), 3 steps (5 ran longer than the termination twin: 148 s against 90 s) of 2 substeps of walk under the 5-term reward, RSI auto-reset, float64; action mode 4 then
    mode 3, each without and with the termination phase (the "deepmimic" fall set and a limit of 3 steps).  The program fails unless every horizon held a
    step taken with carried kinematics, an in-wave re-step of the env that starts in a helpers.many_row_states state, and an auto-reset that a step follows
    (mode 4 then reads the fresh cursor)."""
    exe = HP.build_host("spd_rollout_host.cpp", tmp_path / "spd_rollout_host", testbench=True, sanitize=True, opt=("-O1",))
    n, Tn, nsub, limit = 6, 3, 2, 3
    cm, mc = H.compiled_model(), H.mocap("walk")
    from deepmimic_mujoco_amd.imitation import ImitationSpec
    table, params = ImitationSpec(cm).table_for(mc)[:2]
    idx, q, v, _ws, _c = H.varied_states(n, seed=HC.STATE_SEED)
    mi, mq, mv = HC.many_rows()
    idx[MANY_ENV], q[MANY_ENV], v[MANY_ENV] = mi[0], mq[0], mv[0]
    off = 0.2 * np.random.RandomState(HC.ACTION_SEED).randn(Tn, n, 28)
    act4, act3 = off, mc.data_config[idx][None, :, 7:] + off          # mode 4: offsets from the frame the env is at; mode 3: target poses around the starting frames
    cfg = [n, Tn, nsub, HC.STATE_SEED, T.fall_body_mask("deepmimic"), limit, 1, 3, mc.data_config.shape[0], MANY_ENV]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    # the program's input, in the order its main() reads: the model, the clip, the reward's table and parameters, the run, the states, the actions of both modes
    HP.write_arrays(fin, HP.model_arrays(cm, mc.dt) + [HP.f64(mc.data_config), HP.f64(mc.data_vel), HP.f64(table), HP.f64(params), HP.i32(cfg), HP.f64(q), HP.f64(v),
                                                       HP.i32(idx), HP.f64(act4), HP.f64(act3)])
    t0 = time.time()
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=1500)
    print(r.stdout.strip())
    print("the twin ran %.0f s" % (time.time() - t0))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.fromfile(fout, dtype=np.float64).reshape(2, -1)
    for k, mode in enumerate((4, 3)):
        pre_q, pre_done = out[k][:Tn * n * 35].reshape(Tn, n, 35), out[k][Tn * n * 35:].reshape(Tn, n)
        # the input condition: no fall decision of the step launches' run within rounding of its boundary
        closest = HC.closest_decision(cm, pre_q, pre_done == 0)
        print("mode %d: closest fall decision to its boundary: %.3e m" % (mode, closest))
        assert closest > HC.BOUNDARY
