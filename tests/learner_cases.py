"""The inputs and float64 references of the per-block learner grid (tests/test_gpu_learner_edges.py) — TEST INFRASTRUCTURE, numpy only.

Every case is built on the CPU from a seed, with the float32-rounded numbers the kernels see, and carries its reference; the references are
computed once per process and shared (do not modify what these functions return).  tests/test_learner_blocks.py checks every case on the CPU
— the references against finite differences, `assert_well_scaled`, the constructed minibatches' construction — so a case that cannot carry
the per-block rule is found before any GPU time is spent."""
import functools

import numpy as np

from tests import bc_numpy as BN
from tests import gail_numpy as GN
from tests import learner_blocks as LB
from tests import ppo_numpy as PN
from tests import trpo_numpy as TN
from tests import vf_numpy as VN

f32 = lambda a: np.asarray(a, dtype=np.float32)
f64 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)     # the float32-rounded numbers, as float64

# ---- a. the value fit -------------------------------------------------------------------------------------------------------------------
VF_BS = (1, 31, 32, 33, 96, 160, 2049)                                 # 1, 1, 1, 2, 3, 5 and 65 blocks of 32 samples
VF_NB = 2
VF_CONST_COL, VF_WIDE_COLS = 7, (0, 1)
BETA1, BETA2, ADAM_EPS = (float(np.float32(x)) for x in (0.9, 0.999, 1e-8))      # what the kernels' float arguments hold


def vf_scales(t0, k, stepsize=1e-3):
    return [float(np.float32(stepsize * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))) for t in range(t0 + 1, t0 + 1 + k)]


def vf_rms(c):
    rms = TN.Rms()
    rms.sum, rms.sumsq, rms.count = c["sum0"].copy(), c["sumsq0"].copy(), float(c["count0"])
    return rms


@functools.lru_cache(maxsize=None)
def vf_case(bs):
    """Two minibatches of `bs` rows from a non-zero filter state and non-zero Adam moments.  Column 7 of the observations is constant (its
    std sits on the 0.1 floor), columns 0 and 1 have rows far outside +-5 filter stds (the clip), and the returns sit ~2 above the net's
    values, so that the sum of dy — b3's gradient — does not cancel."""
    rng = np.random.RandomState(1000 + bs)
    n = VF_NB * bs
    scale, shift = np.linspace(0.5, 2.5, 56), rng.randn(56) * 0.4
    draw = lambda k: rng.randn(k, 56) * scale + shift
    prior, ob = draw(200), draw(n)
    for col, sign in zip(VF_WIDE_COLS, (1.0, -1.0)):                   # outliers: the first and the middle row of each minibatch (few: they widen the std too)
        rows = np.unique(np.concatenate([np.arange(0, n, bs), np.arange(bs // 2, n, bs)]))
        ob[rows, col] = shift[col] + sign * 40.0 * scale[col]
    prior[:, VF_CONST_COL] = 0.5; ob[:, VF_CONST_COL] = 0.5
    ob = f32(ob)
    prior = f64(prior)
    sum0, sumsq0, count0 = prior.sum(0), (prior * prior).sum(0), 200.0
    theta0 = f32(np.concatenate([rng.randn(int(np.prod(VN.SHAPES[k]))) * (0.15 if k.endswith("/w") else 0.1) for k in VN.VF]))
    ret = f32(2.0 + rng.randn(n))
    c = dict(bs=bs, nb=VF_NB, ob=ob, ret=ret, theta0=theta0, sum0=sum0, sumsq0=sumsq0, count0=count0, scales=vf_scales(4, VF_NB),
             beta1=BETA1, beta2=BETA2, eps=ADAM_EPS)
    # the Adam moments the epoch starts from: sized by the first minibatch's gradient, block by block, so that the new gradient is most of m
    # (0.1 g against 0.9 m0) and about half of v — an error of the gradient is not hidden behind the state carried in
    rms = vf_rms(c)
    rms.update(ob[:bs])
    g1 = VN.gradient(f64(theta0), VN.normalise(ob[:bs], *VN.published(rms)), f64(ret[:bs]))
    m0, v0 = np.zeros(VN.NP), np.zeros(VN.NP)
    for _, o, k in LB.VALUE:
        top = np.abs(g1[o:o + k]).max()
        m0[o:o + k] = 0.02 * top * rng.randn(k); v0[o:o + k] = 1e-3 * top * top * rng.rand(k)
    c["m0"], c["v0"] = f32(m0), f32(v0)
    c["ref"], c["rms_after"] = vf_reference(c)
    return c


def vf_reference(c, nb=None, dtype=np.float64):
    """-> (fit_epoch's per-minibatch records, the filter after the epoch)"""
    rms = vf_rms(c)
    nb = c["nb"] if nb is None else nb
    rec = VN.fit_epoch(f64(c["theta0"]), f64(c["m0"]), f64(c["v0"]), rms, c["ob"], f64(c["ret"]), nb, c["bs"], c["scales"], c["beta1"], c["beta2"],
                       c["eps"], dtype=dtype)
    return rec, rms


# ---- b. PPO -------------------------------------------------------------------------------------------------------------------------------
PPO_ROWS = 200                                                         # the segment the minibatches are gathered from
PPO_N = (1, 31, 32, 33, 65)
PPO_ENT = 0.01


@functools.lru_cache(maxsize=None)
def ppo_data():
    """tests.test_ppo.problem's segment, reordered so that row 0 takes the unclipped branch with a non-zero advantage (n = 1 must have a
    policy gradient).  -> dict: theta (float64 of the float32 values), mean, std, d (float32 arrays), first [rows] (the branch per row)"""
    from tests.test_ppo import problem
    _, theta, mean, std, d = problem(PPO_ROWS, 7)
    theta = f64(theta)
    d["ret"] = f32(d["ret"] + 1.5)                                     # a mean error of the value net: the sum of dy (vf/b3's gradient) does not cancel
    first = ppo_rows_first(theta, mean, std, d, 0.2)
    k = int(np.flatnonzero(first & (np.abs(d["atarg"]) > 0.3))[0])
    perm = np.arange(PPO_ROWS); perm[[0, k]] = perm[[k, 0]]
    d = {key: (v if key == "old_logstd" else np.ascontiguousarray(v[perm])) for key, v in d.items()}
    return dict(theta=theta, mean=mean, std=std, d=d, first=first[perm])


def ppo_ratio(theta, mean, std, d):
    m = BN.forward(theta[:PN.NPI], mean, std, d["ob"])[3]
    return np.exp(PN.neglogp(f64(d["ac"]), f64(d["old_mean"]), f64(d["old_logstd"])) - PN.neglogp(f64(d["ac"]), m, theta[PN.NPI - 28:PN.NPI]))


def ppo_rows_first(theta, mean, std, d, clip):
    ratio, A = ppo_ratio(theta, mean, std, d), f64(d["atarg"])
    return ratio * A <= np.clip(ratio, 1.0 - clip, 1.0 + clip) * A


def ppo_reference(S, d, rows, clip, ent=PPO_ENT):
    return PN.lossgrad(S["theta"], S["mean"], S["std"], d["ob"][rows], d["ac"][rows], d["atarg"][rows], d["old_mean"][rows], d["old_logstd"],
                       d["ret"][rows], clip, ent)


@functools.lru_cache(maxsize=None)
def ppo_case(n, gathered):
    """rows 0 .. n - 1, or n rows drawn WITH replacement: one row three times inside the first tile, one row in two tiles (n > 32), and for
    n = 1 a row of the unclipped branch.  -> dict(idx (None: rows 0 .. n - 1), rows, ref = (losses, gradient), clip)"""
    S = ppo_data()
    if gathered:
        rng = np.random.RandomState(50 + n)
        rows = rng.randint(0, PPO_ROWS, size=n)
        if n == 1:
            rows[0] = int(np.flatnonzero(S["first"] & (np.abs(S["d"]["atarg"]) > 0.3))[1])
        if n >= 3:
            rows[[0, 7 % n, n - 1 if n <= 32 else 31]] = rows[0]       # three times inside one tile
        if n > 32:
            rows[32] = rows[3]                                         # in two tiles
    else:
        rows = np.arange(n)
    return dict(n=n, idx=rows.astype(np.int32) if gathered else None, rows=rows, clip=0.2, ref=ppo_reference(S, S["d"], rows, 0.2))


@functools.lru_cache(maxsize=None)
def ppo_constructed(kind):
    """Three minibatches of 33 rows (rows 0 .. 32 of a segment of their own, idx = None):
      "clipped"   every row has |ratio - 1| > 2 clip and the minimum takes the clipped branch: old_mean is moved along (ac - mean) until the
                  log-ratio is +-(0.7 .. 1.5) in float64, and atarg gets the sign of (ratio - 1) — the factor 2 keeps float32 from flipping a row;
      "zero_adv"  atarg is zero on every row: every row ties, the gradient flows through the first argument and is zero;
      "clip0"     clip = 0.
    -> dict(d, n, clip, ref, zero: the blocks that are exactly zero by construction)"""
    S = ppo_data()
    n, clip = 33, 0.2
    d = {k: (v.copy() if k == "old_logstd" else v[:n].copy()) for k, v in S["d"].items()}
    zero = ()
    if kind == "clipped":
        rng = np.random.RandomState(11)
        theta = S["theta"]
        m = BN.forward(theta[:PN.NPI], S["mean"], S["std"], d["ob"])[3]
        ls, lo, x = theta[PN.NPI - 28:PN.NPI], f64(d["old_logstd"]), f64(d["ac"])
        target = rng.uniform(0.7, 1.5, n) * np.where(rng.rand(n) < 0.5, -1.0, 1.0)       # log ratio = neglogp_old - neglogp_new
        s_new = (((x - m) / np.exp(ls)) ** 2).sum(1)
        s_old1 = (((x - m) / np.exp(lo)) ** 2).sum(1)                   # with old_mean = x - t (x - m): 0.5 t^2 s_old1 + sum(lo) is neglogp_old (up to the constant)
        t = np.sqrt((2.0 * (target + (ls - lo).sum()) + s_new) / s_old1)
        d["old_mean"] = f32(x - t[:, None] * (x - m))
        ratio = ppo_ratio(theta, S["mean"], S["std"], d)
        d["atarg"] = f32(np.sign(ratio - 1.0) * (0.3 + np.abs(f64(d["atarg"]))))
        zero = tuple("pol/" + k for k in ("W1", "b1", "W2", "b2", "W3", "b3"))
    elif kind == "zero_adv":
        d["atarg"] = np.zeros(n, np.float32)
        zero = tuple("pol/" + k for k in ("W1", "b1", "W2", "b2", "W3", "b3"))
    elif kind == "clip0":
        clip = 0.0
    else:
        raise ValueError(kind)
    return dict(d=d, n=n, clip=clip, zero=zero, ref=ppo_reference(S, d, np.arange(n), clip))


# ---- c. the discriminator -----------------------------------------------------------------------------------------------------------------
DISC_SHAPES = ((1, 1), (32, 32), (31, 33), (33, 31), (1, 65), (65, 1))
DISC_ENT = (1e-3, 1.0)


@functools.lru_cache(maxsize=None)
def disc_case(ng, ne, entcoeff, logit_scale=2.0):
    """a random discriminator and filter, generator rows around the filter's mean and expert rows 0.3 off it (logit_scale 14: logits of
    +-20 .. 30, the saturated regime).  -> dict(theta, mean, std float32; g_ob, g_ac, e_ob, e_ac float32; ref = (losses, gradient))"""
    rng = np.random.RandomState(300 + 7 * ng + ne)
    parts = [rng.randn(int(np.prod(s))) * (0.1 if len(s) == 1 else 0.12) for s in GN.SHAPES]
    parts[4] = rng.randn(100) * 0.12 * logit_scale; parts[5] = 0.8 + rng.randn(1) * 0.2       # (b3 off zero: mean_g s and mean_e (1 - s) do not cancel in b3's gradient)
    theta = f32(np.concatenate(parts))
    mean, std = f32(rng.randn(56) * 0.3), f32(0.5 + rng.rand(56))
    draw = lambda k, off: (f32(mean + off + std * rng.randn(k, 56) * 1.5), f32(rng.randn(k, 28) * 0.8))
    g_ob, g_ac = draw(ng, 0.0)
    e_ob, e_ac = draw(ne, 0.3)
    c = dict(ng=ng, ne=ne, entcoeff=entcoeff, theta=theta, mean=mean, std=std, g_ob=g_ob, g_ac=g_ac, e_ob=e_ob, e_ac=e_ac)
    c["ref"] = disc_reference(c)
    return c


def disc_reference(c, theta=None):
    return GN.lossandgrad(f64(c["theta"]) if theta is None else theta, f64(c["mean"]), f64(c["std"]), f64(c["g_ob"]), f64(c["g_ac"]), f64(c["e_ob"]),
                          f64(c["e_ac"]), c["entcoeff"])


@functools.lru_cache(maxsize=None)
def pg_case(n):
    """dm_pg_losses with write_old = 1 on rows 0 .. n - 1 of the PPO segment -> (the policy's means [n, 28], the gradient of the surrogate
    at pi == oldpi).  That gradient, mean_n atarg_n grad log pi(ac_n), is PPO's unclipped branch with old == new (ratio = 1), negated."""
    S = ppo_data()
    m = BN.forward(S["theta"][:PN.NPI], S["mean"], S["std"], S["d"]["ob"][:n])[3]
    d = {k: (v if k == "old_logstd" else v[:n]) for k, v in S["d"].items()}
    d["old_mean"], d["old_logstd"] = m, S["theta"][PN.NPI - 28:PN.NPI]
    losses, g = ppo_reference(S, d, np.arange(n), 0.2, ent=0.0)
    assert losses[3] == 0.0 and losses[5] == 0.0                       # KL 0, nothing clipped
    return m, -g[:PN.NPI]


# ---- d. the forward kernels ---------------------------------------------------------------------------------------------------------------
ACT_N = (1, 15, 16, 17, 33)
TAIL_N = (1, 31, 33)


@functools.lru_cache(maxsize=None)
def act_case(n):
    """dm_policy_act on n observations: the packed weights (filter, policy, value net — MlpPolicy.pack's order), float64 observations with
    |z| > 5 on some entries, and the float64 forward of both nets on the clipped, normalised observation."""
    S = ppo_data()
    rng = np.random.RandomState(70 + n)
    ob = S["mean"] + S["std"] * rng.randn(n, 56) * 2.5
    packed = f32(np.concatenate([S["mean"], S["std"], S["theta"]]))
    x = np.clip((f64(ob) - S["mean"]) / S["std"], -5.0, 5.0)           # (the kernel rounds the float64 observation to float32 first)
    p = dict(zip(TN.POL, BN.unflatten(S["theta"][:PN.NPI])))
    q = dict(zip(TN.VF, PN.vunflatten(S["theta"][PN.NPI:])))
    mean_ref, _ = TN.pol_forward(p, x)
    v_ref, _ = TN.vf_forward(q, x)
    assert n < 15 or (np.abs(x) == 5.0).any()
    return dict(n=n, ob=ob, packed=packed, mean=mean_ref, vpred=v_ref, sigma=np.exp(p["logstd"].reshape(-1)))
