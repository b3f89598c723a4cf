"""Early termination inside the horizon launch (DM_OPT_HORIZON_TERMINATION; csrc/slot_term.h, csrc/kernels_rollout_term.hip), without a GPU: the
option's id in the header, the Python mirror and both libraries, DPVecEnv's argument errors, and the wave-testbench twin — the kernel source on CPU
fibres under the sanitizers, the horizon with the termination phase inside against step launches followed by k_terminate's own body, bit for bit.
tests/test_gpu_horizon_termination.py has the device."""
import os
import re
import subprocess

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
    assert int(re.search(r"DM_OPT_HORIZON_TERMINATION = (\d+)", hdr).group(1)) == A.OPT_HORIZON_TERMINATION == 12
    assert "unless DM_OPT_HORIZON_TERMINATION" in hdr                  # the paragraph under DM_OPT_MAX_EPISODE_STEPS names the exception
    assert int(re.search(r"#define DM_ABI_VERSION (\d+)", hdr).group(1)) == A.ABI_VERSION == 9      # one id added, no export, nothing moved
    ids = [int(m) for m in re.findall(r"^\s*DM_OPT_[A-Z_]+ = (\d+)", hdr, flags=re.M)]
    assert len(ids) == len(set(ids)) and max(ids) == 12


@pytest.mark.parametrize("dtype", [64, 32])
def test_both_libraries_refuse_the_option_without_a_batch(dtype):
    """an option call is refused on the host where there is no batch (there is no device here: the values a batch accepts and refuses are
    tests/test_gpu_horizon_termination.py's)"""
    L = A.load(dtype)
    for v in (0, 1, 2, -1):
        assert L.dm_batch_set_option(None, A.OPT_HORIZON_TERMINATION, v) == -1 and b"null" in L.dm_last_error()


# ---- the facade -----------------------------------------------------------------------------------------------------------------------------
def test_vec_env_argument_errors_come_before_any_device_call(monkeypatch):
    from deepmimic_mujoco_amd import dp_env

    def no_device(*a, **k):
        raise AssertionError("a batch was created")
    monkeypatch.setattr(dp_env, "Batch", no_device)
    with pytest.raises(ValueError, match="fall_contact_bodies or max_episode_steps"):
        DPVecEnv(8, horizon_termination=True)
    for kw in (dict(action_mode="spd-target"), dict(action_mode="spd-mocap"), dict(obs_mode="deepmimic")):
        with pytest.raises(ValueError, match="no horizon launch"):
            DPVecEnv(8, horizon_termination=True, max_episode_steps=3, fall_contact_bodies="deepmimic", **kw)
    with pytest.raises(AssertionError, match="a batch was created"):   # a valid combination goes on to the batch
        DPVecEnv(8, horizon_termination=True, max_episode_steps=3)


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
    ok = ap.parse_args(["--horizon-termination", "--max-episode-steps", "600", "--fall-contact", "deepmimic"])
    common.check_env_args(ap, ok)
    assert common.env_kwargs(ok)["horizon_termination"] is True and common.env_kwargs(ap.parse_args([]))["horizon_termination"] is False
    for bad in (["--horizon-termination"], ["--horizon-termination", "--max-episode-steps", "5", "--action-mode", "spd-target"],
                ["--horizon-termination", "--fall-contact", "deepmimic", "--obs-mode", "deepmimic"]):
        with pytest.raises(SystemExit):
            common.check_env_args(ap, ap.parse_args(bad))
    assert "--horizon-termination" in capsys.readouterr().err


# ---- the twin on the wave testbench -----------------------------------------------------------------------------------------------------------
def test_horizon_with_termination_equals_step_launches_on_the_wave_testbench(tmp_path):
    """10 envs (two full waves and one with two spare slots), 7 steps of walk under the 5-term reward, RSI auto-reset, the "deepmimic" fall set and a limit
    of 3 steps, float64; then the same with the fall set off and the truncation log on.  The program fails unless the horizon held a fall, a time-limit
    end, a step-own done, a re-step and a truncation record."""
    exe = HP.build_host("term_rollout_host.cpp", tmp_path / "term_rollout_host", testbench=True, sanitize=True, opt=("-O1",))
    n, Tn, limit = 10, 7, 3
    cm, mc = H.compiled_model(), H.mocap("walk")
    from deepmimic_mujoco_amd.imitation import ImitationSpec
    table, params = ImitationSpec(cm).table_for(mc)[:2]
    idx, q, v = HC.states(n)
    act = HC.actions(Tn, n)
    cfg = [n, Tn, 1, HC.STATE_SEED, T.fall_body_mask("deepmimic"), limit, 1, 3, mc.data_config.shape[0]]      # n, T, substeps, seed, fall set, limit, RSI, imitation, frames
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    # the program's input, in the order its main() reads: the model, the clip, the reward's table and parameters, the run, the states, the actions
    HP.write_arrays(fin, HP.model_arrays(cm, mc.dt) + [HP.f64(mc.data_config), HP.f64(mc.data_vel), HP.f64(table), HP.f64(params), HP.i32(cfg), HP.f64(q), HP.f64(v),
                                                       HP.i32(idx), HP.f64(act)])
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=1500)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.fromfile(fout, dtype=np.float64)
    pre_q, pre_done = out[:Tn * n * 35].reshape(Tn, n, 35), out[Tn * n * 35:].reshape(Tn, n)
    # the input condition: no fall decision of the step launches' run within rounding of its boundary
    closest = HC.closest_decision(cm, pre_q, pre_done == 0)
    print("closest fall decision to its boundary: %.3e m" % closest)
    assert closest > HC.BOUNDARY
