"""PPO on the MI355X: dm_ppo_lossgrad (csrc/pg_kernel.h MODE_PPO, csrc/vf_kernel.h k_vf_grad_rows, k_ppo_step) against the float64 numpy
restatement (tests/ppo_numpy.py), dm_ppo_fit against dm_ppo_lossgrad + the Adam rule, ppo.learn's kernel path against its torch path, and
end-to-end runs of tools/train_ppo.py and tools/train_gail.py --algo ppo."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import ppo
from deepmimic_mujoco_amd.trpo import MpiAdam
from tests import learner_blocks as LB
from tests import ppo_numpy as P
from tests.test_policy import CKPT
from tests.test_ppo import problem

DEV = "cuda:0"
NROWS = 9000                                                           # the segment the minibatches are gathered from
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NTH = P.NPI + P.NVF


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def setup():
    pi, theta, mean, std, d = problem(NROWS, 7)
    D = {k: torch.as_tensor(v, device=DEV).contiguous() for k, v in d.items()}
    th = torch.as_tensor(theta.astype(np.float32), device=DEV).contiguous()
    rms = (torch.as_tensor(mean.astype(np.float32), device=DEV), torch.as_tensor(std.astype(np.float32), device=DEV))
    return dict(theta=theta, mean=mean, std=std, d=d, D=D, th=th, rms=rms)


def lossgrad(S, n, idx, clip=0.2, ent=0.0, grad=True, th=None):
    L = A.load()
    th = S["th"] if th is None else th
    scratch = torch.empty(int(L.dm_ppo_scratch_bytes(n if grad else 1)), dtype=torch.uint8, device=DEV)
    out = torch.full((6,), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((NTH,), float("nan"), dtype=torch.float32, device=DEV) if grad else None
    idx_d = torch.as_tensor(idx, dtype=torch.int32, device=DEV) if idx is not None else None
    D = S["D"]
    A.check(L.dm_ppo_lossgrad(_p(D["ob"]), _p(D["ac"]), _p(D["atarg"]), _p(D["old_mean"]), _p(D["old_logstd"]), _p(D["ret"]), _p(idx_d), n, _p(th),
                              _p(S["rms"][0]), _p(S["rms"][1]), clip, ent, _p(g), _p(out), _p(scratch), scratch.numel(), _stream()), L)
    torch.cuda.synchronize()
    return out.cpu().numpy(), (g.cpu().numpy() if grad else None)


def fit(S, th, m, v, idx, scales, clip=0.2, ent=0.0, beta1=0.9, beta2=0.999, eps=1e-5):
    L = A.load()
    iters, bs = idx.shape
    scratch = torch.empty(int(L.dm_ppo_scratch_bytes(bs)), dtype=torch.uint8, device=DEV)
    out = torch.full((iters, 6), float("nan"), dtype=torch.float64, device=DEV)
    idx_d = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int32, device=DEV)
    D = S["D"]
    A.check(L.dm_ppo_fit(_p(D["ob"]), _p(D["ac"]), _p(D["atarg"]), _p(D["old_mean"]), _p(D["old_logstd"]), _p(D["ret"]), _p(idx_d), iters, bs, _p(th),
                         _p(m), _p(v), (C.c_float * iters)(*scales), (C.c_float * iters)(*([clip] * iters)), beta1, beta2, eps, ent, _p(S["rms"][0]),
                         _p(S["rms"][1]), _p(out), _p(scratch), scratch.numel(), _stream()), L)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _scales(t0, k, stepsize=3e-4, beta1=0.9, beta2=0.999):
    return [stepsize * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) for t in range(t0 + 1, t0 + 1 + k)]


def _ref(S, rows, clip=0.2, ent=0.0):
    d = S["d"]
    return P.lossgrad(S["theta"].astype(np.float32).astype(np.float64), S["mean"], S["std"], d["ob"][rows], d["ac"][rows], d["atarg"][rows],
                      d["old_mean"][rows], d["old_logstd"], d["ret"][rows], clip, ent)


@pytest.mark.gpu
@pytest.mark.parametrize("gathered", [False, True])
@pytest.mark.parametrize("n", [64, 1000, 4096])
def test_ppo_lossgrad_matches_numpy(setup, n, gathered):
    rng = np.random.RandomState(n)
    rows = rng.choice(NROWS, n, replace=False) if gathered else np.arange(n)
    ent = 0.01
    losses, g = lossgrad(setup, n, rows if gathered else None, ent=ent)
    ref, gref = _ref(setup, rows, ent=ent)
    assert 0 < ref[5] < 1                                              # rows on both sides of the clip
    for k in range(5):
        assert abs(losses[k] - ref[k]) <= 2e-5 * abs(ref[k]) + 1e-9, (k, losses[k], ref[k])
    assert abs(losses[5] - ref[5]) <= 2.0 / n                          # a row at the clip's edge may count either way in float32
    for lo, hi in ((0, P.NPI), (P.NPI, NTH)):                          # per half: against the half's largest entry
        scale = np.abs(gref[lo:hi]).max()
        assert np.abs(g[lo:hi] - gref[lo:hi]).max() <= 1e-4 * scale, (lo, np.abs(g[lo:hi] - gref[lo:hi]).max(), scale)
    print("ppo n=%d gathered=%d: per block %s" % (n, gathered, LB.block_errors(g, gref, LB.PPO)))
    LB.assert_blocks(g, gref, LB.PPO, LB.BAR, "ppo n=%d" % n)         # ... and per block: against the block's own largest entry
    # the losses alone (no gradient): the same numbers
    lonly, _ = lossgrad(setup, n, rows if gathered else None, ent=ent, grad=False)
    assert np.array_equal(lonly, losses)


@pytest.mark.gpu
def test_ppo_lossgrad_is_bitwise_reproducible(setup):
    rows = np.random.RandomState(1).choice(NROWS, 4096, replace=False)
    a = lossgrad(setup, 4096, rows)
    b = lossgrad(setup, 4096, rows)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [1, 33, 64, 4096])
def test_ppo_fit_one_step_equals_lossgrad_and_adam(setup, bs):
    rng = np.random.RandomState(bs)
    rows = rng.choice(NROWS, bs, replace=False)
    th = setup["th"].clone()
    m = torch.as_tensor(rng.randn(NTH).astype(np.float32) * 1e-3, device=DEV)
    v = torch.as_tensor(rng.rand(NTH).astype(np.float32) * 1e-5, device=DEV)
    losses, g = lossgrad(setup, bs, rows, ent=0.01)
    a = _scales(4, 1)[0]
    gd = torch.as_tensor(g, device=DEV)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)   # the kernel's float32 constants: (1 - beta) is taken in float32
    b1, b2, one = f32(0.9), f32(0.999), f32(1.0)
    m_ref = b1 * m + (one - b1) * gd
    v_ref = b2 * v + (one - b2) * gd * gd
    th_ref = th + (-f32(a)) * m_ref / (torch.sqrt(v_ref) + f32(1e-5))
    out = fit(setup, th, m, v, rows[None, :], [a], ent=0.01)
    assert np.array_equal(out[0], losses)
    for got, want in ((th, th_ref), (m, m_ref), (v, v_ref)):
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert (np.abs(got - want) <= 2 * np.spacing(np.abs(want).astype(np.float32))).all()


@pytest.mark.gpu
def test_ppo_fit_split_calls_are_bitwise_equal(setup):
    rng = np.random.RandomState(3)
    idx = np.stack([rng.choice(NROWS, 256, replace=False) for _ in range(6)])
    runs = []
    for cuts in ((0, 6), (0, 2, 6)):
        th = setup["th"].clone(); m = torch.zeros(NTH, device=DEV); v = torch.zeros(NTH, device=DEV)
        outs = [fit(setup, th, m, v, idx[a:b], _scales(a, b - a)) for a, b in zip(cuts[:-1], cuts[1:])]
        runs.append((th.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), np.concatenate(outs)))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_ppo_fit_200_steps_match_per_minibatch_path(setup):
    rng = np.random.RandomState(4)
    bs, iters = 64, 200
    idx = np.stack([rng.choice(NROWS, bs, replace=False) for _ in range(iters)])
    th = setup["th"].clone(); m = torch.zeros(NTH, device=DEV); v = torch.zeros(NTH, device=DEV)
    out = fit(setup, th, m, v, idx, _scales(0, iters))
    # per minibatch: dm_ppo_lossgrad + trpo.MpiAdam (the multi-rank path's arithmetic)
    w = setup["th"].clone()
    adam = MpiAdam([w], epsilon=1e-5)
    per = []
    for i in range(iters):
        losses, g = lossgrad(setup, bs, idx[i], th=adam.getflat().contiguous())
        adam.update(torch.as_tensor(g, device=DEV), 3e-4)
        per.append(losses)
    assert np.abs(th.cpu().numpy() - w.cpu().numpy()).max() <= 1e-4
    per = np.array(per)
    np.testing.assert_allclose(out[:, :5], per[:, :5], rtol=1e-3, atol=1e-4)
    assert np.abs(out[:, 5] - per[:, 5]).max() <= 1.0 / bs + 1e-12      # clipfrac: a row at the clip's edge may flip
    assert np.array_equal(out[0], per[0])
    assert out[-20:, 2].mean() < out[:20, 2].mean()                    # the value net fits the returns


def _learn(native, iters=2):
    env = DPVecEnv(64, motion="walk", device=0, reward="alive", autoreset="init", seed=2)
    pi = MlpPolicy(device=torch.device(DEV), seed=2); pi.seed(2)
    calls = {"fit": 0, "torch": 0}

    def spy(loc, glob):                                                # count which path the learner takes
        L = loc["learner"]
        if not hasattr(L, "_spied"):
            L._spied = True
            fit0, tl0 = L.kernel_fit, L.torch_lossgrad
            L.kernel_fit = lambda *a, **k: (calls.__setitem__("fit", calls["fit"] + 1), fit0(*a, **k))[1]
            L.torch_lossgrad = lambda *a, **k: (calls.__setitem__("torch", calls["torch"] + 1), tl0(*a, **k))[1]
    hist = ppo.learn(env, pi, timesteps_per_batch=32, max_iters=iters, schedule="constant", optim_epochs=2, optim_batchsize=64, seed=2,
                     native=native, log=None, callback=spy)
    env.close()
    if native is None:
        assert calls == {"fit": 2 * iters, "torch": 0}                 # one dm_ppo_fit call per epoch
    else:
        assert calls["fit"] == 0 and calls["torch"] == iters * (2 * 32 + 1)
    return hist, {k: v.detach().cpu().numpy() for k, v in pi.params.items()}


@pytest.mark.gpu
def test_learn_native_matches_torch_path():
    hk, pk = _learn(None)
    ht, pt = _learn(False)
    keys = ("loss_pol_surr", "loss_vf_loss", "loss_kl", "loss_ent", "ev_tdlam_before")
    for k in keys:                                                     # the first update: the same segment, float32 both ways
        assert abs(hk[0][k] - ht[0][k]) <= 1e-3 * abs(ht[0][k]) + 1e-6, (k, hk[0][k], ht[0][k])
    for h in hk + ht:
        for k in keys + ("loss_pol_entpen", "clipfrac", "EpLenMean"):
            assert np.isfinite(h[k]), (k, h[k])
    assert hk[1]["loss_vf_loss"] == pytest.approx(ht[1]["loss_vf_loss"], rel=5e-2)
    assert hk[1]["loss_ent"] == pytest.approx(ht[1]["loss_ent"], rel=1e-4)
    for k in pk:
        assert np.abs(pk[k] - pt[k]).max() <= 1e-3, k


@pytest.mark.gpu
def test_train_ppo_end_to_end(tmp_path):
    out, ckpt = str(tmp_path / "ppo.json"), str(tmp_path / "ppo-walk")
    env = dict(os.environ)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_ppo.py"), "--envs", "256", "--horizon", "32", "--iters", "3", "--optim-batchsize", "256",
                        "--motion", "walk", "--reward", "alive", "--out", out, "--save", ckpt, "--log-dir", str(tmp_path / "logs")],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hist = json.load(open(out))["history"]
    assert len(hist) == 3
    for h in hist:
        for k in ("loss_pol_surr", "loss_pol_entpen", "loss_vf_loss", "loss_kl", "loss_ent", "clipfrac", "ev_tdlam_before", "EpLenMean"):
            assert np.isfinite(h[k]), (k, h[k])
        assert 0 < h["loss_kl"] < 0.1
    assert os.path.exists(ckpt + ".index") and os.path.exists(str(tmp_path / "logs" / "progress.csv"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_trpo.py"), "--task", "evaluate", "--load-model-path", ckpt,
                        "--number-trajs", "4"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "Average length" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_train_gail_with_ppo(tmp_path):
    from deepmimic_mujoco_amd.trpo import runner
    expert_pi = MlpPolicy.from_tf_checkpoint(CKPT, device=torch.device(DEV)); expert_pi.seed(0)
    env_e = DPVecEnv(8, motion="walk", device=0, reward="alive", autoreset="init", seed=0)
    path = str(tmp_path / "expert.npz")
    runner(env_e, expert_pi, timesteps_per_batch=1024, stochastic_policy=False, log=lambda *a: None, save_sample=path)
    env_e.close()
    out = str(tmp_path / "gail.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_gail.py"), "--expert-path", path, "--algo", "ppo", "--envs", "128",
                        "--horizon", "32", "--iters", "2", "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    hist = json.load(open(out))["history"]
    assert len(hist) == 2
    for h in hist:
        for k in ("loss_pol_surr", "loss_vf_loss", "loss_kl", "generator_loss", "expert_loss", "EpTrueRewMean"):
            assert np.isfinite(h[k]), (k, h[k])
