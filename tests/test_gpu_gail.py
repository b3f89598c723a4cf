"""GAIL on the MI355X: the discriminator kernels (csrc/disc_kernel.h) against the float64 numpy restatement, the rollout's reward_giver
hook, and a short end-to-end run from an expert written by the shipped checkpoint."""
import os

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy, SegmentCollector
from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.gail import ExpertDataset, TransitionClassifier, learn
from tests import gail_numpy as G
from tests import learner_blocks as LB
from tests.test_policy import CKPT

DEV = "cuda:0"


def _random_d(seed, logit_scale=1.0):
    """a discriminator with random parameters and filter (logits spread out to about +-20 .. 30 with logit_scale 14)"""
    rng = np.random.RandomState(seed)
    rg = TransitionClassifier(device=DEV, seed=seed)
    th = rg.theta.cpu().numpy().astype(np.float64)
    th[18600:18700] *= logit_scale
    th[8400:8500] = rng.randn(100) * 0.1; th[18500:18600] = rng.randn(100) * 0.1; th[18700] = rng.randn() * 0.5
    rg.theta.copy_(torch.as_tensor(th, dtype=torch.float32))
    mean = rng.randn(56).astype(np.float32) * 0.3
    std = (0.5 + rng.rand(56)).astype(np.float32)
    rg.obs_rms.mean.copy_(torch.as_tensor(mean)); rg.obs_rms.std.copy_(torch.as_tensor(std))
    return rg, rg.theta.cpu().numpy(), mean.astype(np.float64), std.astype(np.float64)


def _inputs(rng, n, mean, std):
    ob = mean + std * rng.randn(n, 56) * 1.5
    ac = rng.randn(n, 28) * 0.8
    return ob, ac


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4096 * 64, 1, 31, 33, 1000])
def test_disc_reward_matches_numpy(n):
    rng = np.random.RandomState(n)
    rg, th, mean, std = _random_d(1, logit_scale=14.0)
    ob, ac = _inputs(rng, n, mean, std)
    out = torch.full((n,), float("nan"), dtype=torch.float64, device=DEV)
    rg.reward_into(torch.as_tensor(ob, device=DEV), torch.as_tensor(ac, device=DEV), out)
    r = out.cpu().numpy()
    # the numpy reference sees the float32 inputs the kernel sees
    lg = G.forward(th, mean.astype(np.float32), std.astype(np.float32), ob.astype(np.float32), ac.astype(np.float32))[3]
    lo, hi = G.reward_bracket(lg)
    assert np.isfinite(r).all()
    tol = 1e-5 * np.maximum(1.0, np.abs(hi))
    bad = (r < lo - tol) | (r > hi + tol)
    assert not bad.any(), (int(bad.sum()), lg[bad][:5], r[bad][:5], lo[bad][:5], hi[bad][:5])
    if n >= 1000:
        assert lg.max() > 17.5 and lg.min() < -10.0                   # the saturated regime is exercised
        assert np.any(r == np.float32(-np.log(np.float32(1e-8))))


@pytest.mark.gpu
def test_disc_lossgrad_matches_numpy_and_is_reproducible():
    ng, ne = 4099, 1000
    rng = np.random.RandomState(7)
    rg, th, mean, std = _random_d(2, logit_scale=2.0)
    gob, gac = _inputs(rng, ng, mean, std)
    eob, eac = _inputs(rng, ne, mean + 0.3, std)
    f = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)
    losses, g = rg.lossandgrad(f(gob), f(gac), f(eob), f(eac))
    losses2, g2 = rg.lossandgrad(f(gob), f(gac), f(eob), f(eac))
    assert torch.equal(g, g2) and torch.equal(losses, losses2)          # fixed reduction order
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    ref_l, ref_g = G.lossandgrad(th.astype(np.float64), f32(mean), f32(std), f32(gob), f32(gac), f32(eob), f32(eac), 1e-3)
    lk, gk = losses.cpu().numpy(), g.cpu().numpy().astype(np.float64)
    assert np.allclose(lk[:4], ref_l[:4], rtol=1e-4, atol=1e-6), (lk, ref_l)
    assert abs(lk[4] - ref_l[4]) <= 3.0 / ng and abs(lk[5] - ref_l[5]) <= 3.0 / ne   # (a sample on the 0.5 boundary may flip)
    scale = np.abs(ref_g).max()
    assert abs(np.linalg.norm(gk) - np.linalg.norm(ref_g)) <= 1e-4 * np.linalg.norm(ref_g)
    assert np.abs(gk - ref_g).max() <= 1e-4 * scale, np.abs(gk - ref_g).max() / scale
    print("disc 4099, 1000: per block %s" % LB.block_errors(gk, ref_g, LB.DISC))
    LB.assert_blocks(gk, ref_g, LB.DISC, LB.BAR, "disc")               # ... and per block: against the block's own largest entry
    # and the torch path (used where the kernels cannot run) agrees with both
    rg.native = False
    lt, gt = rg.lossandgrad(f(gob), f(gac), f(eob), f(eac))
    assert np.abs(gt.cpu().numpy() - ref_g).max() <= 1e-4 * scale


def _collect(pol, env, rg, T, fused, nseg=2):
    c = SegmentCollector(pol, env, T, stochastic=True, first_reset="init", fused=fused, reward_giver=rg)
    out = []
    for _ in range(nseg):
        c.launch()
        out.append(c.collect())
    return out


@pytest.mark.gpu
def test_segment_with_reward_giver():
    n, T = 256, 32
    rg, _, _, _ = _random_d(3, logit_scale=1.0)
    pol = MlpPolicy.from_tf_checkpoint(CKPT, device=DEV); pol.seed(5)
    env = DPVecEnv(n, motion="walk", device=0, reward="alive", autoreset="init", seed=2)
    segs = _collect(pol, env, rg, T, fused=True, nseg=8)
    env.close()
    for s in segs:
        want = rg.get_reward(s["ob"].reshape(-1, 56), s["ac"].reshape(-1, 28)).reshape(T, n)
        assert torch.equal(s["rew"], want)
        assert len(s["ep_true_rets"]) == len(s["ep_rets"]) == len(s["ep_lens"])
    lens = [x for s in segs for x in s["ep_lens"]]
    assert len(lens) > 0
    # the env's returns are what the same seed gives without a reward_giver (alive reward: the episode length)
    pol2 = MlpPolicy.from_tf_checkpoint(CKPT, device=DEV); pol2.seed(5)
    env2 = DPVecEnv(n, motion="walk", device=0, reward="alive", autoreset="init", seed=2)
    plain = _collect(pol2, env2, None, T, fused=True, nseg=8)
    env2.close()
    for a, b in zip(segs, plain):
        assert a["ep_lens"] == b["ep_lens"] and a["ep_true_rets"] == b["ep_rets"]
        # (two batches may step on different kernels — packed or one-env — whose results differ in the last bits: DM_OPT_PACKED)
        assert torch.allclose(a["ob"], b["ob"], rtol=1e-3, atol=1e-3) and torch.allclose(a["ac"], b["ac"], rtol=1e-3, atol=1e-3)
    assert all(np.isfinite(s["ep_rets"])) and all(r > 0 for r in s["ep_rets"])           # D's returns: sums of positive rewards


@pytest.mark.gpu
def test_reward_giver_in_every_launch_form():
    """The hook is the same whichever way the horizon was stepped — one launch per horizon (dm_batch_rollout), one launch per step
    (DM option 106 = 0), or the policy and the env as separate launches: rew = D(ob, ac) bitwise, the env's returns are the episode
    lengths (alive reward), and the rows every form shares (the first observation and D's reward of it) are identical."""
    n, T = 256, 16
    rg, _, _, _ = _random_d(4, logit_scale=1.0)
    res = []
    for fused, mode in ((True, 1), (True, 0), (False, None)):
        pol = MlpPolicy.from_tf_checkpoint(CKPT, device=DEV); pol.seed(9)
        env = DPVecEnv(n, motion="walk", device=0, reward="alive", autoreset="init", seed=6)
        if mode is not None:
            env.batch.set_option(106, mode)
        segs = _collect(pol, env, rg, T, fused=fused, nseg=3)
        env.close()
        for s in segs:
            assert torch.equal(s["rew"], rg.get_reward(s["ob"].reshape(-1, 56), s["ac"].reshape(-1, 28)).reshape(T, n))
            assert s["ep_true_rets"] == [float(x) for x in s["ep_lens"]] and len(s["ep_rets"]) == len(s["ep_lens"])
        res.append(segs)
    for segs in res[1:]:
        assert torch.equal(segs[0]["ob"][0], res[0][0]["ob"][0]) and torch.equal(segs[0]["rew"][0], res[0][0]["rew"][0])


@pytest.mark.gpu
def test_gail_end_to_end(tmp_path):
    dev = torch.device(DEV)
    # the expert: the shipped checkpoint, deterministic, written through runner(save_sample=...) (= train_trpo.py --save-sample)
    from deepmimic_mujoco_amd.trpo import runner
    expert_pi = MlpPolicy.from_tf_checkpoint(CKPT, device=dev); expert_pi.seed(0)
    env_e = DPVecEnv(16, motion="walk", device=0, reward="alive", autoreset="init", seed=0)
    path = str(tmp_path / "expert.npz")
    runner(env_e, expert_pi, timesteps_per_batch=1024, stochastic_policy=False, log=lambda *a: None, save_sample=path)
    env_e.close()
    expert = ExpertDataset(path, seed=0, device=dev)
    assert expert.num_traj == 16 and expert.num_transition > 16 * 100
    env = DPVecEnv(256, motion="walk", device=0, reward="alive", autoreset="init", seed=1)
    pi = MlpPolicy(device=dev, seed=1); pi.seed(1)
    rg = TransitionClassifier(device=dev, seed=1)
    theta0 = rg.theta.clone()
    hist = learn(env, pi, rg, expert, g_step=3, d_step=1, timesteps_per_batch=32, max_iters=3, log=None, seed=1)
    assert len(hist) == 3
    for h in hist:
        for k in ("generator_loss", "expert_loss", "entropy", "entropy_loss", "generator_acc", "expert_acc", "meankl", "surrgain", "EpTrueRewMean"):
            assert np.isfinite(h[k]), (k, h[k])
    assert not torch.equal(theta0, rg.theta) and bool(torch.isfinite(rg.theta).all())
    # with the policy fixed, a few D updates separate the policy's transitions from the expert's
    from deepmimic_mujoco_amd.trpo import MpiAdam
    from deepmimic_mujoco_amd.rollout import traj_segment_generator
    adam = MpiAdam([rg.theta])
    gen = traj_segment_generator(pi, env, 32, stochastic=True, fused=True, reward_giver=rg)
    seg = next(gen)
    ob, ac = seg["ob"].reshape(-1, 56), seg["ac"].reshape(-1, 28)
    for _ in range(50):
        eob, eac = expert.get_next_batch(ob.shape[0])
        rg.obs_rms.update(torch.cat([ob, eob], 0))
        losses, g = rg.lossandgrad(ob, ac, eob, eac)
        adam.update(g, 3e-4)
    losses = rg.lossandgrad(ob, ac, *expert.get_next_batch(ob.shape[0]))[0].tolist()
    env.close()
    assert losses[4] > 0.5 and losses[5] > 0.5, losses
