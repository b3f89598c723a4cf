"""Behaviour cloning on the MI355X: dm_bc_lossgrad (csrc/pg_kernel.h MODE_BC) against the float64 numpy restatement (tests/bc_numpy.py),
dm_bc_fit against dm_bc_lossgrad + the Adam rule, and BC from an expert written by the shipped checkpoint, followed by GAIL."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy
from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import behavior_clone as BC
from deepmimic_mujoco_amd.gail import ExpertDataset, TransitionClassifier, learn
from deepmimic_mujoco_amd.trpo import POL_KEYS, VF_KEYS, MpiAdam
from tests import bc_numpy as N
from tests import learner_blocks as LB
from tests.test_behavior_clone import random_policy
from tests.test_policy import CKPT

DEV = "cuda:0"
NROWS = 70000                                                          # the expert set the batches are gathered from


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _expert(seed=0):
    rng = np.random.RandomState(seed)
    ob = rng.randn(NROWS, 56).astype(np.float32)
    ob[:, :6] *= 12.0                                                  # |z| > 5 on some entries: the clip is exercised
    ac = (rng.randn(NROWS, 28) * 0.5).astype(np.float32)
    return ob, ac, torch.as_tensor(ob, device=DEV), torch.as_tensor(ac, device=DEV)


@pytest.fixture(scope="module")
def setup():
    pi, theta, mean, std = random_policy(3, device=DEV)
    ob, ac, ob_d, ac_d = _expert()
    th = torch.as_tensor(theta, device=DEV).contiguous()
    return dict(pi=pi, theta=theta, mean=mean, std=std, ob=ob, ac=ac, ob_d=ob_d, ac_d=ac_d, th=th)


def lossgrad(S, n, idx, stochastic, seed, counter, grad=True, th=None):
    L = A.load()
    th = S["th"] if th is None else th
    scratch = torch.empty(int(L.dm_bc_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((th.numel(),), float("nan"), dtype=torch.float32, device=DEV) if grad else None
    idx_d = torch.as_tensor(idx, dtype=torch.int32, device=DEV) if idx is not None else None
    rms = S["pi"].ob_rms
    A.check(L.dm_bc_lossgrad(_p(S["ob_d"]), _p(S["ac_d"]), _p(idx_d), n, _p(th), _p(rms.mean), _p(rms.std), stochastic, seed, counter, _p(g), _p(loss),
                             _p(scratch), scratch.numel(), _stream()), L)
    torch.cuda.synchronize()
    return float(loss.item()), (g.cpu().numpy() if grad else None)


def fit(S, th, m, v, idx, scales, seed, counter0, beta1=0.9, beta2=0.999, eps=1e-5):
    L = A.load()
    iters, bs = idx.shape
    scratch = torch.empty(int(L.dm_bc_scratch_bytes(bs)), dtype=torch.uint8, device=DEV)
    out = torch.full((iters,), float("nan"), dtype=torch.float64, device=DEV)
    idx_d = torch.as_tensor(np.ascontiguousarray(idx), dtype=torch.int32, device=DEV)
    rms = S["pi"].ob_rms
    sc = (C.c_float * iters)(*scales)
    A.check(L.dm_bc_fit(_p(S["ob_d"]), _p(S["ac_d"]), _p(idx_d), iters, bs, _p(th), _p(m), _p(v), sc, beta1, beta2, eps, _p(rms.mean), _p(rms.std), 1,
                        seed, counter0, _p(out), _p(scratch), scratch.numel(), _stream()), L)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _scales(t0, k, stepsize=3e-4, beta1=0.9, beta2=0.999):
    return [stepsize * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t) for t in range(t0 + 1, t0 + 1 + k)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 128, 4096, 65536])
def test_bc_lossgrad_matches_numpy(setup, n):
    S = setup
    rng = np.random.RandomState(n)
    for gathered in (False, True):
        idx = rng.randint(0, NROWS, size=n).astype(np.int32) if gathered else None
        rows = idx if gathered else np.arange(n)
        ob, ac = S["ob"][rows], S["ac"][rows]
        for stochastic in (0, 1):
            eps = N.noise(7, 12345, n, bool(stochastic))
            lref, gref = N.lossgrad(S["theta"].astype(np.float64), S["mean"], S["std"], ob, ac, eps)
            loss, g = lossgrad(S, n, idx, stochastic, 7, 12345)
            # the loss: float32 forward (three layers, ~1e-6 relative), float32 Box-Muller against float64 (~1e-6), per-sample sums of 28
            # squares in float32, everything past the tile in float64
            assert abs(loss - lref) <= 2e-5 * lref, (gathered, stochastic, loss, lref)
            # the gradient: float32 MFMA sums over up to 256 rows per block (error ~ sqrt(rows) ulp of the sum of |terms|), float32 partials
            # added over up to 256 blocks: held to 1e-4 of the gradient's largest entry
            assert np.isfinite(g).all()
            err = np.abs(g - gref).max() / np.abs(gref).max()
            assert err <= 1e-4, (gathered, stochastic, err)
            print("bc n=%d gathered=%d stochastic=%d: per block %s" % (n, gathered, stochastic, LB.block_errors(g, gref, LB.POLICY)))
            LB.assert_well_scaled(gref, LB.POLICY, exempt=() if stochastic else ("logstd",))
            LB.assert_blocks(g, gref, LB.POLICY, LB.BAR, "bc n=%d gathered=%d stochastic=%d" % (n, gathered, stochastic))      # every block against its own largest entry
            if stochastic:
                ls = np.abs(gref[-28:]).max()
                assert np.abs(g[-28:] - gref[-28:]).max() <= 1e-4 * ls
            else:
                assert not g[-28:].any()                                # the mode: logstd has no gradient
            loss_only, none = lossgrad(S, n, idx, stochastic, 7, 12345, grad=False)
            assert loss_only == loss and none is None


@pytest.mark.gpu
def test_bc_lossgrad_is_bitwise_reproducible(setup):
    idx = np.random.RandomState(1).randint(0, NROWS, size=4096)
    a = lossgrad(setup, 4096, idx, 1, 3, 9)
    b = lossgrad(setup, 4096, idx, 1, 3, 9)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    c = lossgrad(setup, 4096, idx, 1, 3, 10)                           # another counter: other noise
    assert c[0] != a[0]


@pytest.mark.gpu
@pytest.mark.parametrize("bs", [128, 1000])
def test_bc_fit_one_step_equals_lossgrad_and_adam(setup, bs):
    S = setup
    idx = np.random.RandomState(bs).randint(0, NROWS, size=(1, bs)).astype(np.int32)
    loss, g = lossgrad(S, bs, idx[0], 1, 5, 40)
    th = S["th"].clone(); m = torch.zeros_like(th); v = torch.zeros_like(th)
    out = fit(S, th, m, v, idx, _scales(0, 1), 5, 40)
    assert out[0] == loss                                              # the same sums in the same order
    f = np.float32
    a = f(_scales(0, 1)[0])
    mm = f(0.9) * f(0) + f(1 - f(0.9)) * g
    vv = f(0.999) * f(0) + f(1 - f(0.999)) * g * g
    want = S["theta"] + (-a) * mm / (np.sqrt(vv) + f(1e-5))
    np.testing.assert_array_max_ulp(m.cpu().numpy(), mm.astype(np.float32), maxulp=2)
    np.testing.assert_array_max_ulp(v.cpu().numpy(), vv.astype(np.float32), maxulp=2)
    np.testing.assert_array_max_ulp(th.cpu().numpy(), want.astype(np.float32), maxulp=2)


@pytest.mark.gpu
def test_bc_fit_split_calls_are_bitwise_equal(setup):
    S = setup
    K, bs = 25, 128
    idx = np.random.RandomState(3).randint(0, NROWS, size=(2 * K, bs)).astype(np.int32)
    th1 = S["th"].clone(); m1 = torch.zeros_like(th1); v1 = torch.zeros_like(th1)
    l1 = fit(S, th1, m1, v1, idx, _scales(0, 2 * K), 11, 100)
    th2 = S["th"].clone(); m2 = torch.zeros_like(th2); v2 = torch.zeros_like(th2)
    la = fit(S, th2, m2, v2, idx[:K], _scales(0, K), 11, 100)
    lb = fit(S, th2, m2, v2, idx[K:], _scales(K, K), 11, 100 + K)
    assert np.array_equal(l1, np.concatenate([la, lb]))
    assert torch.equal(th1, th2) and torch.equal(m1, m2) and torch.equal(v1, v2)
    assert not torch.equal(th1, S["th"])


@pytest.mark.gpu
def test_bc_fit_loss_curve_matches_per_iteration_path(setup):
    """200 iterations: dm_bc_fit against dm_bc_lossgrad + MpiAdam (the multi-rank path of behavior_clone.learn, on one process)."""
    S = setup
    iters, bs = 200, 128
    idx = np.random.RandomState(4).randint(0, NROWS, size=(iters, bs)).astype(np.int32)
    th = S["th"].clone(); m = torch.zeros_like(th); v = torch.zeros_like(th)
    fused = fit(S, th, m, v, idx, _scales(0, iters), 2, 0)
    p = S["th"].clone()
    adam = MpiAdam([p], epsilon=1e-5)
    per = []
    for it in range(iters):
        loss, g = lossgrad(S, bs, idx[it], 1, 2, it, th=p)
        adam.update(torch.as_tensor(g, device=DEV), 3e-4)
        per.append(loss)
    per = np.array(per)
    assert np.abs(fused - per).max() <= 1e-4 * np.abs(per).max(), np.abs(fused - per).max()
    assert fused[-20:].mean() < fused[:20].mean()
    assert (th - p).abs().max().item() <= 1e-4 * p.abs().max().item()


@pytest.mark.gpu
def test_learn_native_matches_torch_path_and_keeps_value_net(setup):
    """learn() through dm_bc_fit against learn() through torch autograd on the same GPU, from the same policy and expert draws."""
    data = {"obs": setup["ob"][:6000].reshape(20, 300, 56), "acs": np.tanh(setup["ob"][:6000, :28] * 0.1).reshape(20, 300, 28), "rets": np.zeros(20)}
    res = []
    for native in (True, False):
        pi = random_policy(3, device=DEV)[0]
        before = {k: v.detach().clone() for k, v in pi.params.items()}
        e = ExpertDataset(data, seed=0, device=DEV)
        train, val = BC.learn(pi, e, max_iters=300, verbose=True, native=native, chunk=64, log=None)
        for k in VF_KEYS:
            assert torch.equal(pi.params[k], before[k])
        res.append((train, val, torch.cat([pi.params[k].detach().reshape(-1) for k in POL_KEYS])))
    (t1, v1, p1), (t2, v2, p2) = res
    assert [i for i, _ in v1] == [i for i, _ in v2] == list(range(0, 300, 30))
    assert np.abs(t1 - t2).max() <= 1e-3 * np.abs(t2).max()
    assert np.allclose([x for _, x in v1], [x for _, x in v2], rtol=1e-3)
    assert (p1 - p2).abs().max().item() <= 1e-2 * p2.abs().max().item()           # (Adam's normalised steps amplify float32 noise where g ~ 0)


@pytest.mark.gpu
def test_bc_then_gail_end_to_end(tmp_path):
    dev = torch.device(DEV)
    from deepmimic_mujoco_amd.trpo import runner
    expert_pi = MlpPolicy.from_tf_checkpoint(CKPT, device=dev); expert_pi.seed(0)
    env_e = DPVecEnv(16, motion="walk", device=0, reward="alive", autoreset="init", seed=0)
    path = str(tmp_path / "expert.npz")
    runner(env_e, expert_pi, timesteps_per_batch=1024, stochastic_policy=False, log=lambda *a: None, save_sample=path)
    env_e.close()
    expert = ExpertDataset(path, seed=0, device=dev)
    pi = MlpPolicy(device=dev, seed=1); pi.seed(1)
    ls0 = pi.params["logstd"].detach().clone()
    vf0 = {k: pi.params[k].detach().clone() for k in VF_KEYS}
    lines = []
    train, val = BC.learn(pi, expert, max_iters=2000, verbose=True, seed=1, log=lines.append)
    assert [i for i, _ in val] == list(range(0, 2000, 200)) and len(lines) == 10
    v = [x for _, x in val]
    print("BC val losses:", " ".join("%.4f" % x for x in v), "ratio %.3f" % (v[-1] / v[0]))
    assert np.isfinite(train).all() and np.isfinite(v).all()
    assert v[-1] <= 0.35 * v[0], v                                       # (measured: 0.224 of the first val loss; seeded and bitwise reproducible)
    assert float(pi.params["logstd"].mean()) < float(ls0.mean())
    for k in VF_KEYS:
        assert torch.equal(pi.params[k], vf0[k])
    prefix = str(tmp_path / "bc")
    pi.save_tf_checkpoint(prefix)
    back = MlpPolicy.from_tf_checkpoint(prefix, device=dev)
    for k, x in pi.state_dict().items():
        assert np.array_equal(np.asarray(x).reshape(-1), np.asarray(back.state_dict()[k]).reshape(-1)), k
    env = DPVecEnv(256, motion="walk", device=0, reward="alive", autoreset="init", seed=1)
    rg = TransitionClassifier(device=dev, seed=1)
    hist = learn(env, pi, rg, expert, g_step=1, d_step=1, timesteps_per_batch=32, max_iters=2, log=None, seed=1)
    env.close()
    assert len(hist) == 2
    for h in hist:
        for k in ("generator_loss", "expert_loss", "meankl", "surrgain", "EpTrueRewMean"):
            assert np.isfinite(h[k]), (k, h[k])
