"""GAIL without a GPU: the discriminator's torch path against the float64 numpy restatement (tests/gail_numpy.py), ExpertDataset and the
rollout's reward_giver bookkeeping against the reference's own code (tests/golden/gail_ref_golden.npz, tests/golden/gen/make_gail_fixture.py),
the --save-sample writer, and the host-side checks of the new C ABI entry points."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import MlpPolicy, SegmentCollector
from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.gail import LOSS_NAMES, ExpertDataset, TransitionClassifier
from deepmimic_mujoco_amd.trpo import runner
from tests import gail_numpy as G

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gail_ref_golden.npz")


def _d(seed=0, logit_scale=1.0):
    rng = np.random.RandomState(seed)
    rg = TransitionClassifier(seed=seed)
    th = rg.theta.numpy().astype(np.float64)
    th[18600:18700] *= logit_scale
    th[8400:8500] = rng.randn(100) * 0.1; th[18500:18600] = rng.randn(100) * 0.1; th[18700] = rng.randn() * 0.3
    rg.theta.copy_(torch.as_tensor(th, dtype=torch.float32))
    ob = rng.randn(300, 56) * 2 + 0.5
    rg.obs_rms.update(torch.as_tensor(ob))
    return rg, rng


def test_parameter_layout_and_init():
    rg = TransitionClassifier(seed=3)
    assert rg.theta.numel() == 18701 == 84 * 100 + 100 + 100 * 100 + 100 + 100 + 1
    w1, b1, w2, b2, w3, b3 = rg.unflatten()
    for w, fan in ((w1, 184), (w2, 200), (w3, 101)):                  # Glorot-uniform bounds, zero biases
        lim = np.sqrt(6.0 / fan)
        assert float(w.abs().max()) <= lim and float(w.abs().max()) > 0.9 * lim
    assert float(b1.abs().sum() + b2.abs().sum() + b3.abs().sum()) == 0.0
    d = rg.state_dict()
    assert d["adversary/fully_connected/weights"].shape == (84, 100) and d["adversary/fully_connected_2/weights"].shape == (100, 1)
    assert float(d["adversary/obfilter/count"]) == 1e-2


def test_forward_and_reward_match_numpy():
    rg, rng = _d(1, logit_scale=14.0)
    ob = rng.randn(2000, 56) * 2; ac = rng.randn(2000, 28)
    mean, std = rg.obs_rms.mean.numpy().astype(np.float64), rg.obs_rms.std.numpy().astype(np.float64)
    ob32, ac32 = ob.astype(np.float32).astype(np.float64), ac.astype(np.float32).astype(np.float64)
    lg_np = G.forward(rg.theta.numpy(), mean, std, ob32, ac32)[3]
    lg = rg.logits(torch.as_tensor(ob), torch.as_tensor(ac)).numpy()
    assert np.abs(lg - lg_np).max() <= 1e-5 * max(1.0, np.abs(lg_np).max())
    assert lg_np.max() > 17.5                                          # saturated rows are in the batch
    r = rg.get_reward(ob, ac).numpy()
    assert r.shape == (2000, 1) and r.dtype == np.float32
    lo, hi = G.reward_bracket(lg_np)
    tol = 1e-5 * np.maximum(1.0, hi)
    assert ((r[:, 0] >= lo - tol) & (r[:, 0] <= hi + tol)).all()
    sat = np.float32(-np.log(np.float32(1e-8)))
    assert np.any(r[:, 0] == sat) and r.max() == sat                   # -log(1e-8): not softplus(logit), which would keep growing
    assert np.isclose(float(rg.get_reward(ob[0], ac[0]).reshape(())), float(r[0, 0]), rtol=1e-5, atol=1e-6)   # a single transition is a batch of one


def test_lossandgrad_matches_numpy_with_unequal_batches():
    rg, rng = _d(2, logit_scale=2.0)
    ng, ne = 157, 61
    gob, gac = rng.randn(ng, 56) * 2, rng.randn(ng, 28)
    eob, eac = rng.randn(ne, 56) * 2 + 0.4, rng.randn(ne, 28) * 0.5
    f = lambda a: torch.as_tensor(a, dtype=torch.float32)
    losses, g = rg.lossandgrad(f(gob), f(gac), f(eob), f(eac))
    assert losses.shape == (6,) and len(LOSS_NAMES) == 6 and g.shape == (18701,)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    mean, std = rg.obs_rms.mean.numpy().astype(np.float64), rg.obs_rms.std.numpy().astype(np.float64)
    ref_l, ref_g = G.lossandgrad(rg.theta.numpy().astype(np.float64), mean, std, f32(gob), f32(gac), f32(eob), f32(eac), rg.entcoeff)
    assert np.allclose(losses.numpy()[:4], ref_l[:4], rtol=1e-5, atol=1e-7)
    assert np.allclose(losses.numpy()[4:], ref_l[4:], atol=1.5 / ne)
    assert abs(ref_l[3] + rg.entcoeff * ref_l[2]) < 1e-12
    scale = np.abs(ref_g).max()
    assert np.abs(g.numpy() - ref_g).max() <= 1e-5 * scale
    # the gradient is the total loss's: a finite difference along it agrees
    th0 = rg.theta.clone()
    eps = 1e-3
    dvec = ref_g / np.linalg.norm(ref_g)

    def total(th):
        ll = G.lossandgrad(th, mean, std, f32(gob), f32(gac), f32(eob), f32(eac), rg.entcoeff)[0]
        return ll[0] + ll[1] + ll[3]
    th64 = th0.numpy().astype(np.float64)
    fd = (total(th64 + eps * dvec) - total(th64 - eps * dvec)) / (2 * eps)
    assert abs(fd - np.linalg.norm(ref_g)) <= 1e-4 * np.linalg.norm(ref_g)
    with pytest.raises(ValueError):
        rg.lossandgrad(f(gob), f(gac), f(eob[:0]), f(eac[:0]))


def test_state_dict_round_trip(tmp_path):
    rg, _ = _d(4)
    p = str(tmp_path / "adv.npz")
    rg.save_npz(p)
    back = TransitionClassifier.from_npz(p)
    assert torch.equal(back.theta, rg.theta) and torch.equal(back.obs_rms.mean, rg.obs_rms.mean) and torch.equal(back.obs_rms.std, rg.obs_rms.std)


# ---- ExpertDataset = Mujoco_Dset --------------------------------------------------------------------------------------------------
def _expert_dict(g, name, key="ep_rets"):
    lens = g[name + "_lens"]
    obs, acs = g[name + "_obs"], g[name + "_acs"]
    if name == "dense":
        O, Ac = obs.reshape(len(lens), lens[0], 56), acs.reshape(len(lens), lens[0], 28)
    else:
        cuts = np.cumsum(lens)[:-1]
        O = np.empty(len(lens), dtype=object); Ac = np.empty(len(lens), dtype=object)
        for i, (o, a) in enumerate(zip(np.split(obs, cuts), np.split(acs, cuts))):
            O[i] = o; Ac[i] = a
    return {"obs": O, "acs": Ac, "lens": lens, key: g[name + "_rets"]}


@pytest.mark.parametrize("name", ["dense", "ragged"])
@pytest.mark.parametrize("seed,tl", [(3, -1), (11, 2)])
@pytest.mark.parametrize("key", ["ep_rets", "rets"])
def test_expert_dataset_matches_reference_batches(name, seed, tl, key):
    g = np.load(GOLD)
    ds = ExpertDataset(_expert_dict(g, name, key), traj_limitation=tl, seed=seed)
    tag = "%s_s%d_tl%d" % (name, seed, tl)
    meta = g[tag + "_meta"]
    assert (ds.num_traj, ds.num_transition) == (int(meta[0]), int(meta[1]))
    assert np.isclose(ds.avg_ret, meta[2]) and np.isclose(ds.std_ret, meta[3])
    rows, o = g[tag + "_batch_rows"], 0
    for b, want_len in zip(g["dset_sizes"], g[tag + "_batch_lens"]):
        ob, ac = ds.get_next_batch(int(b))
        assert ob.shape == (want_len, 56) and ac.shape == (want_len, 28)
        want = rows[o:o + want_len]; o += want_len
        assert np.array_equal(ob[:, 0].numpy().astype(np.int64), want) and np.array_equal(ac[:, 0].numpy().astype(np.int64), want)
        assert np.array_equal(ob.numpy(), g[name + "_obs"][want].astype(np.float32))
    assert any(lb < b for lb, b in zip(g[tag + "_batch_lens"], g["dset_sizes"]))      # a batch larger than the set came back short


# ---- the --save-sample writer ------------------------------------------------------------------------------------------------
class _HostEnv(object):
    """a CPU stand-in with the DPVecEnv calls runner() makes: env e ends its trajectory after 5 + 3 e steps"""

    def __init__(self, n):
        self.num_envs, self.t = n, 0

    def _ob(self):
        return np.sin(0.1 * np.arange(56)[None, :] + 0.5 * np.arange(self.num_envs)[:, None] + 0.07 * self.t)

    def reset(self, mode, out=None):
        self.t = 0
        out[...] = self._ob()

    def step(self, ac):
        self.t += 1
        done = self.t >= 5 + 3 * np.arange(self.num_envs)
        return self._ob(), np.full(self.num_envs, 1.0) + 0.1 * np.arange(self.num_envs), done.astype(np.uint8)


@pytest.mark.parametrize("n", [1, 3])
def test_save_sample_writes_what_expert_dataset_reads(tmp_path, n):
    pi = MlpPolicy(seed=0)
    path = str(tmp_path / "sample.npz")
    avg_len, avg_ret, lens, rets = runner(_HostEnv(n), pi, timesteps_per_batch=100, log=lambda *a: None, save_sample=path)
    assert list(lens) == [5 + 3 * e for e in range(n)]
    f = np.load(path, allow_pickle=True)
    assert sorted(f.files) == ["acs", "ep_rets", "lens", "obs", "rets"]
    assert np.array_equal(f["rets"], f["ep_rets"]) and np.array_equal(f["lens"], lens)
    assert (f["obs"].dtype == object) == (n > 1)                      # unequal lengths: object arrays, as np.array(list) makes them
    ds = ExpertDataset(path, randomize=False)
    assert ds.num_traj == n and ds.num_transition == int(lens.sum())
    ob, ac = ds.get_next_batch(-1)
    env = _HostEnv(n)
    first = np.empty((n, 56)); env.reset("init", out=first)
    assert np.allclose(ob[:1].numpy(), first[:1].astype(np.float32))  # trajectory 0 starts at env 0's first observation
    with torch.no_grad():
        a0 = pi.act(False, torch.as_tensor(first))[0].numpy()
    assert np.allclose(ac[0].numpy(), a0[0].astype(np.float32), atol=1e-6)
    ds2 = ExpertDataset(path, traj_limitation=1)
    assert ds2.num_transition == int(lens[0])


# ---- the rollout's reward_giver bookkeeping against src/gail.py traj_segment_generator ----------------------------------------------
def _standin_reward(ob, ac):
    """= make_gail_fixture.standin_reward (the stand-in discriminator the fixture was made with)"""
    return np.float32(0.3 * np.sin(np.sum(ob) * 0.5) + 0.05 * np.sum(ac) + 1.0)


class _StandInD(object):
    def reward_into(self, ob64, ac64, out64):
        ob, ac = ob64.reshape(-1, 56).numpy(), ac64.reshape(-1, 28).numpy().astype(np.float32)
        out64.copy_(torch.as_tensor([float(_standin_reward(o, a)) for o, a in zip(ob, ac)], dtype=torch.float64).reshape(out64.shape))


class _NoEnv(object):
    num_envs = 1

    def reset(self, mode, out=None):
        pass


def test_reward_giver_segments_match_reference_generator():
    g = np.load(GOLD)
    T, K = (int(x) for x in g["gen_T"])
    c = SegmentCollector(MlpPolicy(seed=0), _NoEnv(), T, device="cpu", reward_giver=_StandInD())
    rets, true_rets, lens = [], [], []
    for k in range(K):
        sl = slice(k * T, (k + 1) * T)
        c.ob64[:T, 0] = torch.as_tensor(g["gen_ob"][sl]); c.ac64[:T, 0] = torch.as_tensor(g["gen_ac"][sl].astype(np.float64))
        c.rew64[:, 0] = torch.as_tensor(g["gen_true_rew"][sl]); c.done8[:, 0] = torch.as_tensor(g["gen_done"][sl])
        seg = c.collect()
        assert np.array_equal(seg["rew"][:, 0].numpy(), g["gen_rew"][k])               # D's reward per step (gail.py:78)
        assert len(seg["ep_rets"]) == len(seg["ep_true_rets"]) == len(seg["ep_lens"]) == int(g["gen_ep_counts"][k])
        rets += seg["ep_rets"]; true_rets += seg["ep_true_rets"]; lens += seg["ep_lens"]
    assert lens == list(g["gen_ep_lens"])
    assert np.allclose(true_rets, g["gen_ep_true_rets"], rtol=1e-12)
    assert np.allclose(rets, g["gen_ep_rets"], rtol=1e-5)             # (the reference sums D's float32 rewards in float32)


def test_no_reward_giver_leaves_segments_as_they_were():
    g = np.load(GOLD)
    T = int(g["gen_T"][0])
    c = SegmentCollector(MlpPolicy(seed=0), _NoEnv(), T, device="cpu")
    c.rew64[:, 0] = torch.as_tensor(g["gen_true_rew"][:T]); c.done8[:, 0] = torch.as_tensor(g["gen_done"][:T])
    seg = c.collect()
    assert "ep_true_rets" not in seg and not hasattr(c, "drew64")
    assert np.array_equal(seg["rew"][:, 0].numpy(), g["gen_true_rew"][:T].astype(np.float32))


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_disc_abi_validates_arguments(dtype):
    L = A.load(dtype)
    assert L.dm_disc_param_count() == 18701
    assert L.dm_disc_scratch_bytes(4099, 1000) == (129 + 32) * 18752 * 4 and L.dm_disc_scratch_bytes(0, 5) == 0
    buf = np.zeros(64, dtype=np.float32)                               # host memory: never dereferenced — every call below is refused first
    p = C.c_void_p(buf.ctypes.data)
    off = C.c_void_p(buf.ctypes.data + 4)                              # theta must be 16-byte aligned (float4 loads)
    assert L.dm_disc_reward(None, p, p, p, p, 8, p, None) == -1 and b"dm_disc_reward" in L.dm_last_error()
    assert L.dm_disc_reward(p, p, p, p, p, 0, p, None) == -1
    assert L.dm_disc_reward(off, p, p, p, p, 8, p, None) == -1
    args = lambda ng, ne, sb, th=p, ent=1e-3: (th, p, p, p, p, ng, p, p, ne, ent, p, p, p, sb, None)
    big = L.dm_disc_scratch_bytes(64, 64)
    assert L.dm_disc_lossgrad(*args(0, 4, big)) == -1
    assert L.dm_disc_lossgrad(*args(4, 0, big)) == -1
    assert L.dm_disc_lossgrad(*args(64, 64, big - 1)) == -1 and b"scratch" in L.dm_last_error()
    assert L.dm_disc_lossgrad(*args(4, 4, big, th=off)) == -1
    assert L.dm_disc_lossgrad(*args(4, 4, big, ent=float("nan"))) == -1
    if not torch.cuda.is_available():                                  # well-formed calls without a device: a clean error, no CPU path
        assert L.dm_disc_reward(p, p, p, p, p, 8, p, None) == -5 and b"no HIP device" in L.dm_last_error()
        assert L.dm_disc_lossgrad(*args(4, 4, big)) == -5 and b"no HIP device" in L.dm_last_error()
