"""PPO without a GPU: the float64 numpy restatement (tests/ppo_numpy.py) against finite differences, the torch path of
deepmimic_mujoco_amd.ppo against it, the minibatch bookkeeping of one update (steps per epoch, the dropped tail, a fresh permutation per
epoch, lrmult on both step and clip), a zero step size, and the host-side checks of dm_ppo_scratch_bytes / dm_ppo_lossgrad / dm_ppo_fit."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import MlpPolicy
from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import ppo
from deepmimic_mujoco_amd.trpo import POL_KEYS, VF_KEYS
from tests import ppo_numpy as P
from tests.test_behavior_clone import random_policy


def problem(n, seed, clip=0.2, spread=0.4):
    """a random policy + value net and a batch whose old means sit off the current ones (ratios on both sides of the clip, A of both signs)
    -> (pi, theta [pol + vf] float64, mean, std, dict of numpy arrays)"""
    pi, theta_pi, mean, std = random_policy(seed)
    rng = np.random.RandomState(seed + 100)
    with torch.no_grad():
        for k in VF_KEYS:
            pi.params[k].copy_(torch.as_tensor(rng.randn(*pi.params[k].shape) * (0.15 if k.endswith("/w") else 0.1), dtype=torch.float32))
    theta_vf = torch.cat([pi.params[k].detach().reshape(-1) for k in VF_KEYS]).numpy()
    ob = rng.randn(n, 56).astype(np.float32)
    ob[:, :6] *= 12.0                                                  # |z| > 5 on some entries: the clip of the observation is exercised
    m = P.BN.forward(theta_pi.astype(np.float64), mean, std, ob)[3]
    ls = theta_pi[-28:].astype(np.float64)
    ac = (m + np.exp(ls) * rng.randn(n, 28)).astype(np.float32)
    old_mean = (m + spread * np.exp(ls) * rng.randn(n, 28) / np.sqrt(28)).astype(np.float32)
    old_logstd = (ls + 0.05 * rng.randn(28)).astype(np.float32)
    atarg = rng.randn(n).astype(np.float32)
    ret = rng.randn(n).astype(np.float32)
    theta = np.concatenate([theta_pi, theta_vf]).astype(np.float64)
    return pi, theta, mean, std, dict(ob=ob, ac=ac, atarg=atarg, old_mean=old_mean, old_logstd=old_logstd, ret=ret)


def np_args(d):
    return d["ob"], d["ac"], d["atarg"], d["old_mean"], d["old_logstd"], d["ret"]


def test_numpy_gradient_matches_finite_differences():
    pi, theta, mean, std, d = problem(40, 1)
    clip, ent = 0.2, 0.01
    losses, g = P.lossgrad(theta, mean, std, *np_args(d), clip, ent)
    assert g.shape == (P.NPI + P.NVF,) and P.NPI == 18656 and P.NVF == 15901
    # the batch covers both branches of min() with both signs of A
    m = P.BN.forward(theta[:P.NPI], mean, std, d["ob"])[3]
    ratio = np.exp(P.neglogp(d["ac"], d["old_mean"], d["old_logstd"].astype(np.float64)) - P.neglogp(d["ac"], m, theta[P.NPI - 28:P.NPI]))
    A_ = d["atarg"].astype(np.float64)
    clipped = np.clip(ratio, 1 - clip, 1 + clip) * A_ < ratio * A_
    assert clipped.any() and (~clipped).any()
    assert (clipped & (A_ < 0)).any() and (clipped & (A_ > 0)).any()
    assert 0 < losses[5] < 1 and losses[3] > 0
    rng = np.random.RandomState(2)
    shapes = P.BN.SHAPES + P.VSHAPES
    offs = np.cumsum([0] + [int(np.prod(s)) for s in shapes])
    picks = [o + k for o, e in zip(offs[:-1], offs[1:]) for k in rng.choice(e - o, min(5, e - o), replace=False)]
    for i in picks:
        h = 1e-6
        tp, tm = theta.copy(), theta.copy(); tp[i] += h; tm[i] -= h
        fd = (P.total_loss(tp, mean, std, *np_args(d), clip, entcoeff=ent) - P.total_loss(tm, mean, std, *np_args(d), clip, entcoeff=ent)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-7 + 1e-5 * abs(g[i]), (i, fd, g[i])


def _double(pi):
    for k in POL_KEYS + VF_KEYS:
        pi.params[k] = pi.params[k].detach().to(torch.float64)
    return pi


def _torch_batch(d, dtype):
    return {k: torch.as_tensor(v).to(dtype) for k, v in d.items()}


@pytest.mark.parametrize("n", [1, 33, 200])
@pytest.mark.parametrize("entcoeff", [0.0, 0.01])
def test_torch_lossgrad_matches_numpy(n, entcoeff):
    pi, theta, mean, std, d = problem(n, 10 + n)
    L = ppo.PpoLearner(_double(pi), entcoeff=entcoeff, schedule="constant", native=False)
    D = _torch_batch(d, torch.float64)
    rows = torch.from_numpy(np.random.RandomState(n).permutation(n)[:max(1, n - 3)])
    losses, g = L.torch_lossgrad(D, rows, 0.2)
    r = rows.numpy()
    ref, gref = P.lossgrad(theta, mean, std, d["ob"][r], d["ac"][r], d["atarg"][r], d["old_mean"][r], d["old_logstd"], d["ret"][r], 0.2, entcoeff)
    np.testing.assert_allclose(losses.numpy(), ref, rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(g.numpy(), gref, rtol=1e-6, atol=1e-9 * np.abs(gref).max())


def _update_problem(n=200, seed=3, **kw):
    pi = MlpPolicy(seed=seed)
    rng = np.random.RandomState(seed)
    ob = torch.as_tensor(rng.randn(n, 56).astype(np.float32))
    ac = torch.as_tensor(rng.randn(n, 28).astype(np.float32))
    adv = torch.as_tensor(rng.randn(n).astype(np.float32))
    ret = torch.as_tensor(rng.randn(n).astype(np.float32))
    vpred = torch.as_tensor(rng.randn(n).astype(np.float32))
    kw.setdefault("native", False)
    return pi, ppo.PpoLearner(pi, **kw), (ob, ac, adv, ret, vpred)


def test_minibatch_bookkeeping():
    n, bs, epochs = 200, 64, 3
    pi, L, batch = _update_problem(n, optim_batchsize=bs, optim_epochs=epochs, schedule="linear", max_timesteps=1000)
    L.timesteps_so_far = 250                                           # lrmult = 0.75
    perms, rows_seen, clips, steps = [], [], [], []
    gen = torch.Generator().manual_seed(5)

    def perm_source(k):
        p = torch.randperm(k, generator=gen)
        perms.append(p.clone())
        return p
    L.perm_source = perm_source
    orig_lg, orig_up = L.torch_lossgrad, L.adam.update

    def lg(D, rows, clip, grad=True):
        rows_seen.append((rows.clone() if rows is not None else None, grad)); clips.append(clip)
        return orig_lg(D, rows, clip, grad)

    def up(g, stepsize):
        steps.append(stepsize)
        return orig_up(g, stepsize)
    L.torch_lossgrad, L.adam.update = lg, up
    stats = L.update_batch(*batch)
    nb = n // bs                                                       # 3 minibatches per epoch, the last 8 rows of each shuffle dropped
    assert len(perms) == epochs + 1 and len(steps) == nb * epochs and L.adam.t == nb * epochs
    assert all(not torch.equal(perms[0], p) for p in perms[1:])        # a fresh permutation per epoch (and for the loss pass)
    for e in range(epochs):
        for k in range(nb):
            rows, grad = rows_seen[e * nb + k]
            assert grad and torch.equal(rows, perms[e][k * bs:(k + 1) * bs])
    rows, grad = rows_seen[-1]
    assert not grad and torch.equal(rows, perms[-1][:nb * bs])         # the loss pass: the full minibatches of one more shuffle, no step
    assert clips == [pytest.approx(0.2 * 0.75)] * len(clips)
    assert steps == [pytest.approx(3e-4 * 0.75)] * len(steps)
    assert stats["lrmult"] == pytest.approx(0.75) and stats["optim_steps"] == nb * epochs
    for k in ("loss_pol_surr", "loss_pol_entpen", "loss_vf_loss", "loss_kl", "loss_ent", "clipfrac", "ev_tdlam_before"):
        assert np.isfinite(stats[k]), k
    L.timesteps_so_far = 2000                                          # past max_timesteps: lrmult = 0
    assert L.lrmult() == 0.0


def test_batch_size_none_is_the_whole_batch_and_constant_schedule():
    pi, L, batch = _update_problem(50, optim_batchsize=None, optim_epochs=2, schedule="constant")
    stats = L.update_batch(*batch)
    assert L.adam.t == 2 and stats["lrmult"] == 1.0 and stats["optim_steps"] == 2
    with pytest.raises(ValueError):
        ppo.PpoLearner(MlpPolicy(seed=0), schedule="linear")           # a linear schedule needs max_timesteps


def test_zero_stepsize_leaves_parameters_and_gives_zero_kl():
    pi, L, batch = _update_problem(192, optim_batchsize=64, optim_epochs=2, optim_stepsize=0.0, schedule="constant")
    before = {k: v.detach().clone() for k, v in pi.params.items()}
    count = pi.ob_rms.count.clone()
    stats = L.update_batch(*batch)
    for k in POL_KEYS + VF_KEYS:
        assert torch.equal(pi.params[k], before[k]), k
    assert stats["loss_kl"] == 0.0 and stats["clipfrac"] == 0.0
    assert float(pi.ob_rms.count) == float(count) + 192               # the filter moved once, with the whole batch
    assert stats["loss_pol_surr"] == pytest.approx(-float(((batch[2] - batch[2].mean()) / batch[2].std(unbiased=False)).mean()), abs=1e-6)


def test_update_moves_both_nets_and_follows_the_advantage():
    pi, L, batch = _update_problem(256, optim_batchsize=64, optim_epochs=4, schedule="constant")
    before = {k: v.detach().clone() for k, v in pi.params.items()}
    stats = L.update_batch(*batch)
    for k in POL_KEYS + VF_KEYS:
        assert not torch.equal(pi.params[k], before[k]), k
    assert stats["loss_kl"] > 0 and stats["loss_pol_surr"] < 0          # the surrogate gained on the batch it was fitted to
    assert stats["loss_ent"] == pytest.approx(float((pi.params["logstd"].detach() + 0.5 * np.log(2 * np.pi * np.e)).sum()), rel=1e-6)


@pytest.mark.parametrize("dtype", [64, 32])
def test_ppo_abi_validates_arguments(dtype):
    L = A.load(dtype)
    npad_p = (P.NPI + 63) // 64 * 64
    npad_v = (P.NVF + 63) // 64 * 64
    up = lambda x: (x + 255) // 256 * 256
    assert L.dm_ppo_scratch_bytes(0) == 0 and L.dm_ppo_scratch_bytes(-3) == 0
    assert L.dm_ppo_scratch_bytes(64) == up(256 * 4 * 8) + up(256 * 8) + up(2 * npad_p * 4) + up(2 * npad_v * 4)
    assert L.dm_ppo_scratch_bytes(65536) == up(256 * 4 * 8) + up(2048 * 8) + up(256 * npad_p * 4) + up(2048 * npad_v * 4)
    buf = np.zeros(64, dtype=np.float32)                               # host memory: never dereferenced — every call below is refused first
    p = C.c_void_p(buf.ctypes.data)
    off = C.c_void_p(buf.ctypes.data + 4)                              # theta must be 16-byte aligned (float4 loads)
    big = L.dm_ppo_scratch_bytes(64)
    small = L.dm_ppo_scratch_bytes(1)

    def lg(n=64, sb=big, th=p, ob=p, ret=p, out=p, g=p, clip=0.2, ent=0.0):
        return L.dm_ppo_lossgrad(ob, p, p, p, p, ret, None, n, th, p, p, clip, ent, g, out, p, sb, None)
    assert lg(0) == -1 and b"dm_ppo_lossgrad" in L.dm_last_error()
    assert lg(ob=None) == -1 and lg(ret=None) == -1 and lg(out=None) == -1
    assert lg(th=off) == -1
    assert lg(clip=float("nan")) == -1 and lg(clip=-0.1) == -1 and lg(ent=float("inf")) == -1
    assert lg(sb=big - 1) == -1 and b"scratch" in L.dm_last_error()
    assert lg(n=65, sb=big) == -1                                      # a gradient of 65 rows needs more than 64 rows' scratch
    assert lg(2 ** 31 - 1, sb=2 ** 40) == -1
    scale = (C.c_float * 4)(1e-4, 1e-4, 1e-4, 1e-4)
    clips = (C.c_float * 4)(0.2, 0.2, 0.2, 0.2)
    bad = (C.c_float * 4)(1e-4, float("inf"), 1e-4, 1e-4)
    badclip = (C.c_float * 4)(0.2, -0.2, 0.2, 0.2)

    def fit(iters=4, bs=64, sb=big, th=p, sc=scale, cl=clips, b1=0.9, b2=0.999, eps=1e-5, m=p, ent=0.0):
        return L.dm_ppo_fit(p, p, p, p, p, p, None, iters, bs, th, m, p, sc, cl, b1, b2, eps, ent, p, p, p, p, sb, None)
    assert fit(iters=0) == -1 and b"dm_ppo_fit" in L.dm_last_error()
    assert fit(bs=0) == -1 and fit(m=None) == -1 and fit(sc=None) == -1 and fit(cl=None) == -1
    assert fit(th=off) == -1
    assert fit(sb=big - 1) == -1 and b"scratch" in L.dm_last_error()
    assert fit(b1=float("nan")) == -1 and fit(eps=float("inf")) == -1 and fit(ent=float("nan")) == -1
    assert fit(sc=bad) == -1 and b"step scale" in L.dm_last_error()
    assert fit(cl=badclip) == -1
    if not torch.cuda.is_available():                                  # well-formed calls without a device: a clean error, no CPU path
        assert lg() == -5 and b"no HIP device" in L.dm_last_error()
        assert lg(n=100000, sb=small, g=None) == -5                    # losses alone: dm_ppo_scratch_bytes(1) suffices for any n
        assert fit() == -5 and b"no HIP device" in L.dm_last_error()
