"""The value bootstrap at a time-limit end, without a GPU: the float64 restatement of the rule (tests/gae_numpy.py) against the
reference-generated GAE fixture, the torch fallback of `add_vtarg_and_adv` with a "vboot" key against the restatement, a closed form, and the ABI of
the truncation log (DM_OPT_TRUNCATION_LOG, dm_batch_truncations, dm_gae_boot).  tests/test_gpu_truncation.py has the kernels."""
import os
import re

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.rollout import add_vtarg_and_adv
from tests.gae_numpy import gae_boot, random_segment

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
G = np.load(os.path.join(ROOT, "tests", "golden", "learner_ref_golden.npz"))
RTOL, ATOL = 2e-5, 2e-4            # tests/test_learner_reference.py's for GAE


def as_torch(seg):
    return {k: torch.from_numpy(np.array(v)) for k, v in seg.items()}


def test_restatement_without_bootstrap_equals_the_references_gae():
    gamma, lam = (float(v) for v in G["gae_gamma_lam"])
    for vboot in (None, np.zeros_like(G["gae_rew"])):
        adv, ret = gae_boot(G["gae_rew"], G["gae_vpred"], G["gae_new"], G["gae_nextvpred"], vboot, gamma, lam)
        assert np.allclose(adv, G["gae_adv"], rtol=RTOL, atol=ATOL) and np.allclose(ret, G["gae_tdlamret"], rtol=RTOL, atol=ATOL)
    assert float(np.abs(G["gae_adv"]).max()) > 10


@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("n", [1, 5])
def test_torch_fallback_with_vboot_equals_the_restatement(T, n):
    gamma, lam = 0.99, 0.95
    seg = random_segment(T, n, seed=100 * T + n)
    assert np.count_nonzero(seg["vboot"]) > 0
    want_adv, want_ret = gae_boot(seg["rew"], seg["vpred"], seg["new"], seg["nextvpred"], seg["vboot"], gamma, lam)
    got = add_vtarg_and_adv(as_torch(seg), gamma, lam)
    assert got["adv"].dtype == torch.float32 and tuple(got["adv"].shape) == (T, n)
    assert np.allclose(got["adv"].numpy(), want_adv, rtol=RTOL, atol=ATOL) and np.allclose(got["tdlamret"].numpy(), want_ret, rtol=RTOL, atol=ATOL)
    # the bootstrap is in the numbers: without it the targets differ by gamma * vboot at least at the last row
    plain_adv, _ = gae_boot(seg["rew"], seg["vpred"], seg["new"], seg["nextvpred"], None, gamma, lam)
    assert np.abs(want_adv - plain_adv).max() > 0.5
    # the same call without the key returns today's numbers: the restatement without bootstrap, and bit for bit what a zero vboot gives
    no_key = {k: v for k, v in seg.items() if k != "vboot"}
    plain = add_vtarg_and_adv(as_torch(no_key), gamma, lam)
    assert np.allclose(plain["adv"].numpy(), plain_adv, rtol=RTOL, atol=ATOL)
    zero = add_vtarg_and_adv(as_torch(dict(no_key, vboot=np.zeros((T, n), dtype=np.float32))), gamma, lam)
    assert torch.equal(zero["adv"], plain["adv"]) and torch.equal(zero["tdlamret"], plain["tdlamret"])


def test_without_the_key_the_fixture_still_holds():
    seg = as_torch({"rew": G["gae_rew"], "vpred": G["gae_vpred"], "new": G["gae_new"], "nextvpred": G["gae_nextvpred"]})
    add_vtarg_and_adv(seg, *(float(v) for v in G["gae_gamma_lam"]))
    assert "vboot" not in seg and np.allclose(seg["adv"].numpy(), G["gae_adv"], rtol=RTOL, atol=ATOL)


def test_closed_form_at_lambda_zero():
    """lambda = 0: the advantage is the one-step error, so at every truncated row adv[t] = rew[t] + gamma * vboot[t] - vpred[t] (the episode ends
    there: new[t+1] = 1, or the row is the last and nextvpred is 0 as the collector's rule makes it)."""
    gamma = 0.97
    seg = random_segment(7, 5, seed=3)
    seg["nextvpred"][:] = 0.0                                             # vpreds[T] * (1 - done[-1]) with a done last row
    trunc = seg["vboot"] != 0
    assert trunc.sum() >= 3
    want = seg["rew"].astype(np.float64) + gamma * seg["vboot"].astype(np.float64) - seg["vpred"].astype(np.float64)
    got = add_vtarg_and_adv(as_torch(seg), gamma, 0.0)["adv"].numpy()
    ref, _ = gae_boot(seg["rew"], seg["vpred"], seg["new"], seg["nextvpred"], seg["vboot"], gamma, 0.0)
    assert np.allclose(got[trunc], want[trunc], rtol=RTOL, atol=ATOL) and np.allclose(ref[trunc], want[trunc], rtol=1e-12, atol=1e-12)


def test_phase_of_on_tensors_equals_the_numpy_form():
    from deepmimic_mujoco_amd.state_features import phase_of
    idx = np.array([0, 3, 37, 38, 75], dtype=np.int32); init = np.array([5, 0, 2, 37, 1], dtype=np.int32)
    for mode in range(5):
        got = phase_of(mode, torch.from_numpy(idx), torch.from_numpy(init), 38)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), phase_of(mode, idx, init, 38))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_and_python_mirror_agree():
    hdr = open(os.path.join(ROOT, "include", "dmenv.h")).read()
    assert int(re.search(r"DM_OPT_TRUNCATION_LOG = (\d+)", hdr).group(1)) == A.OPT_TRUNCATION_LOG == 11
    assert "int dm_batch_truncations(" in hdr and "int dm_gae_boot(" in hdr
    assert int(re.search(r"#define DM_ABI_VERSION (\d+)", hdr).group(1)) == A.ABI_VERSION == 9      # one function and one id added, nothing moved


@pytest.mark.parametrize("dtype", [64, 32])
def test_both_libraries_export_and_refuse_bad_arguments(dtype):
    """refused on the host, before any device is touched (there is none here)"""
    import ctypes as C
    L = A.load(dtype)
    for name in ("dm_batch_truncations", "dm_gae_boot"):
        assert name in A.EXPORTS and hasattr(L, name)
    cnt = np.zeros(1, dtype=np.int32)
    assert L.dm_batch_truncations(None, C.c_void_p(cnt.ctypes.data), None, None, None, 0, 0, A.PTR_HOST) == -1 and b"null" in L.dm_last_error()
    assert L.dm_batch_set_option(None, A.OPT_TRUNCATION_LOG, -1) == -1
    x = np.zeros(4, dtype=np.float32); p = C.c_void_p(x.ctypes.data)
    assert L.dm_gae_boot(p, p, p, p, None, p, p, 1, 1, 0.99, 0.95, None) == -1 and b"dm_gae_boot" in L.dm_last_error()       # no vboot
    assert L.dm_gae_boot(p, p, p, p, p, p, p, 0, 1, 0.99, 0.95, None) == -1                                                 # T <= 0


def test_train_tools_refuse_the_flag_without_a_time_limit(capsys):
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import _train_common as common
    finally:
        sys.path.pop(0)
    ap = argparse.ArgumentParser()
    common.add_env_args(ap, reward_help="r")
    ok = ap.parse_args(["--bootstrap-time-limit", "--max-episode-steps", "600"])
    common.check_env_args(ap, ok)
    assert ok.bootstrap_time_limit and not ap.parse_args([]).bootstrap_time_limit
    with pytest.raises(SystemExit):
        common.check_env_args(ap, ap.parse_args(["--bootstrap-time-limit"]))
    assert "--max-episode-steps" in capsys.readouterr().err
