"""Behaviour cloning without a GPU: the float64 numpy restatement (tests/bc_numpy.py) against finite differences, the torch path of
deepmimic_mujoco_amd.behavior_clone against it, what learn() must leave untouched (value net, obs filter, the expert's later shuffles),
the val schedule, a train split smaller than the batch, and the host-side checks of dm_bc_scratch_bytes / dm_bc_lossgrad / dm_bc_fit."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import MlpPolicy
from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import behavior_clone as BC
from deepmimic_mujoco_amd.gail import ExpertDataset
from deepmimic_mujoco_amd.trpo import POL_KEYS, VF_KEYS
from tests import bc_numpy as N


def expert_data(n_traj=4, length=60, seed=0):
    """transitions whose actions are a smooth function of the observations (something a policy can fit)"""
    rng = np.random.RandomState(seed)
    obs = rng.randn(n_traj, length, 56).astype(np.float32)
    w = rng.randn(56, 28) * 0.2
    acs = np.tanh(obs.astype(np.float64) @ w).astype(np.float32)
    return {"obs": obs, "acs": acs, "rets": rng.rand(n_traj) * 100}


def random_policy(seed, device="cpu"):
    """a policy with O(1) weights, a non-trivial logstd and obs filter; -> (pi, flat theta float32, mean, std)"""
    rng = np.random.RandomState(seed)
    pi = MlpPolicy(device=device, seed=seed)
    with torch.no_grad():
        for k in POL_KEYS:
            pi.params[k].copy_(torch.as_tensor(rng.randn(*pi.params[k].shape) * (0.15 if k.endswith("/w") else 0.1), dtype=torch.float32))
        pi.params["logstd"].copy_(torch.as_tensor(rng.randn(1, 28) * 0.3 - 0.5, dtype=torch.float32))
    mean = (rng.randn(56) * 0.3).astype(np.float32)
    std = (0.3 + rng.rand(56)).astype(np.float32)
    pi.ob_rms.mean.copy_(torch.as_tensor(mean)); pi.ob_rms.std.copy_(torch.as_tensor(std))
    theta = torch.cat([pi.params[k].detach().reshape(-1) for k in POL_KEYS]).cpu().numpy()
    return pi, theta, mean.astype(np.float64), std.astype(np.float64)


def batch(rng, n, wide=True):
    ob = rng.randn(n, 56).astype(np.float32)
    if wide:                                                           # |z| > 5 on some entries: the clip is exercised
        ob[:, :6] *= 12.0
    ac = (rng.randn(n, 28) * 0.5).astype(np.float32)
    return ob, ac


def test_numpy_gradient_matches_finite_differences():
    pi, theta, mean, std = random_policy(1)
    rng = np.random.RandomState(2)
    ob, ac = batch(rng, 9)
    eps = N.noise(5, 3, 9)
    th = theta.astype(np.float64)
    _, g = N.lossgrad(th, mean, std, ob, ac, eps)
    assert g.shape == (N.NP,) and N.NP == 18656
    offs = np.cumsum([0] + [int(np.prod(s)) for s in N.SHAPES])
    picks = [o + k for o, e in zip(offs[:-1], offs[1:]) for k in rng.choice(e - o, 6, replace=False)]
    for i in picks:
        h = 1e-6
        tp, tm = th.copy(), th.copy(); tp[i] += h; tm[i] -= h
        fd = (N.loss(tp, mean, std, ob, ac, eps) - N.loss(tm, mean, std, ob, ac, eps)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-7 + 1e-5 * abs(g[i]), (i, fd, g[i])


def test_host_noise_mirror_matches_numpy_restatement():
    idx = np.arange(4096, dtype=np.uint64)
    for seed, counter in ((0, 0), (7, 1), (2 ** 63 + 5, 2 ** 40 + 3)):
        a = BC.normal_from(seed, counter, idx); b = N.normal_from(seed, counter, idx)
        assert np.array_equal(a, b)
    e = N.normal_from(3, 9, np.arange(200000, dtype=np.uint64))
    assert abs(e.mean()) < 0.01 and abs(e.std() - 1.0) < 0.01


@pytest.mark.parametrize("stochastic", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 128])
def test_torch_lossgrad_matches_numpy(n, stochastic):
    pi, theta, mean, std = random_policy(10 + n)
    rng = np.random.RandomState(n)
    ob, ac = batch(rng, n)
    z = (ob - mean) / std
    assert (np.abs(z) > 5).any() and (np.abs(z) < 5).any()
    loss, g = BC._torch_lossgrad(pi, torch.as_tensor(ob), torch.as_tensor(ac), 11, 4, stochastic=bool(stochastic))
    eps = N.noise(11, 4, n, bool(stochastic))
    lref, gref = N.lossgrad(theta.astype(np.float64), mean, std, ob, ac, eps)
    # float32 forward through three layers: ~1e-6 relative on the loss; the gradient is compared against its own scale
    assert abs(float(loss) - lref) <= 1e-5 * lref
    scale = np.abs(gref).max()
    assert np.abs(g.numpy() - gref).max() <= 2e-5 * scale
    assert (np.abs(gref[-28:]) > 0).all() == bool(stochastic)          # logstd is trained only through the stochastic action


def _learn_cpu(pi, expert, **kw):
    kw.setdefault("log", None)
    return BC.learn(pi, expert, native=False, **kw)


def test_learn_leaves_value_net_and_filter_untouched_and_moves_logstd():
    pi = MlpPolicy(seed=3)
    expert = ExpertDataset(expert_data(), seed=0)
    before = {k: v.detach().clone() for k, v in pi.params.items()}
    rms = (pi.ob_rms.sum.clone(), pi.ob_rms.sumsq.clone(), pi.ob_rms.count.clone(), pi.ob_rms.mean.clone(), pi.ob_rms.std.clone())
    pi._dirty = False
    train, val = _learn_cpu(pi, expert, max_iters=300)
    assert train.shape == (300,) and np.isfinite(train).all() and val == []
    for k in VF_KEYS:
        assert torch.equal(pi.params[k], before[k]), k
    for a, b in zip(rms, (pi.ob_rms.sum, pi.ob_rms.sumsq, pi.ob_rms.count, pi.ob_rms.mean, pi.ob_rms.std)):
        assert torch.equal(a, b)
    for k in POL_KEYS:
        assert not torch.equal(pi.params[k], before[k]), k
    assert float(pi.params["logstd"].mean()) < float(before["logstd"].mean())   # the expert is deterministic: sigma shrinks
    assert train[-50:].mean() < 0.8 * train[:50].mean()
    assert pi._dirty


def test_val_schedule():
    for iters, want in ((25, list(range(0, 25, 2))), (10, list(range(10))), (5, list(range(5)))):
        pi = MlpPolicy(seed=0)
        lines = []
        train, val = BC.learn(pi, ExpertDataset(expert_data(), seed=1), max_iters=iters, verbose=True, native=False, log=lines.append)
        assert [it for it, _ in val] == want
        assert len(lines) == len(want) and all(np.isfinite(v) for _, v in val)


def test_expert_draws_after_bc_match_the_draws_without_it():
    draws = []
    for pretrain in (False, True):
        e = ExpertDataset(expert_data(), seed=4)
        if pretrain:
            _learn_cpu(MlpPolicy(seed=0), e, max_iters=40, optim_batch_size=64, verbose=True)
        draws.append([e.next_indices(100).copy() for _ in range(8)])
    for a, b in zip(*draws):
        assert np.array_equal(a, b)


def test_train_split_smaller_than_the_batch():
    e = ExpertDataset(expert_data(n_traj=2, length=10), seed=0)        # 20 transitions: 14 train, 6 val
    sizes = []
    orig = e.next_indices

    def spy(bs, split=None):
        out = orig(bs, split)
        if split == "train":
            sizes.append(len(out))
        return out
    e.next_indices = spy
    train, _ = _learn_cpu(MlpPolicy(seed=0), e, max_iters=12, optim_batch_size=128)
    assert sizes == [14] * 12 and np.isfinite(train).all()


@pytest.mark.parametrize("dtype", [64, 32])
def test_bc_abi_validates_arguments(dtype):
    L = A.load(dtype)
    assert L.dm_pg_param_count() == N.NP
    npad = (N.NP + 63) // 64 * 64
    assert L.dm_bc_scratch_bytes(0) == 0
    assert L.dm_bc_scratch_bytes(128) == (4 * npad * 4 + 255) // 256 * 256 + 4 * 16
    assert L.dm_bc_scratch_bytes(65536) == (256 * npad * 4 + 255) // 256 * 256 + 256 * 16        # one block per CU at most
    buf = np.zeros(64, dtype=np.float32)                               # host memory: never dereferenced — every call below is refused first
    p = C.c_void_p(buf.ctypes.data)
    off = C.c_void_p(buf.ctypes.data + 4)                              # theta must be 16-byte aligned (float4 loads)
    big = L.dm_bc_scratch_bytes(64)
    lg = lambda n, sb=big, th=p, ob=p, out=p: (ob, p, None, n, th, p, p, 1, 0, 0, None, out, p, sb, None)
    assert L.dm_bc_lossgrad(*lg(0)) == -1 and b"dm_bc_lossgrad" in L.dm_last_error()
    assert L.dm_bc_lossgrad(*lg(8, ob=None)) == -1
    assert L.dm_bc_lossgrad(*lg(8, out=None)) == -1
    assert L.dm_bc_lossgrad(*lg(8, th=off)) == -1
    assert L.dm_bc_lossgrad(*lg(64, sb=big - 1)) == -1 and b"scratch" in L.dm_last_error()
    assert L.dm_bc_lossgrad(*lg(2 ** 31 - 1, sb=2 ** 40)) == -1
    scale = (C.c_float * 4)(1e-4, 1e-4, 1e-4, 1e-4)
    bad = (C.c_float * 4)(1e-4, float("inf"), 1e-4, 1e-4)

    def fit(iters=4, bs=64, sb=big, th=p, sc=scale, b1=0.9, b2=0.999, eps=1e-5, m=p):
        return L.dm_bc_fit(p, p, None, iters, bs, th, m, p, sc, b1, b2, eps, p, p, 1, 0, 0, p, p, sb, None)
    assert fit(iters=0) == -1 and b"dm_bc_fit" in L.dm_last_error()
    assert fit(bs=0) == -1
    assert fit(m=None) == -1
    assert fit(sc=None) == -1
    assert fit(th=off) == -1
    assert fit(bs=64, sb=big - 1) == -1 and b"scratch" in L.dm_last_error()
    assert fit(b1=float("nan")) == -1 and fit(eps=float("inf")) == -1
    assert fit(sc=bad) == -1 and b"step scale" in L.dm_last_error()
    if not torch.cuda.is_available():                                  # well-formed calls without a device: a clean error, no CPU path
        assert L.dm_bc_lossgrad(*lg(8)) == -5 and b"no HIP device" in L.dm_last_error()
        assert fit() == -5 and b"no HIP device" in L.dm_last_error()
