"""float64 numpy restatement of one PPO minibatch (OpenAI baselines' ppo1 `pposgd_simple`), written from its formulas: the policy mean and
the value net of src/mlp_policy_trpo.py (clip of the normalised observation included), DiagGaussianPd's neglogp / kl / entropy
(src/distributions.py), the clipped surrogate with TF's tie-break of `minimum`, and the flat gradient of pol_surr + pol_entpen + vf_loss
over both nets by hand-written backpropagation.  The tests hold deepmimic_mujoco_amd.ppo (torch path) and the kernels to it."""
import numpy as np

from tests import bc_numpy as BN

OB, H, AC = 56, 100, 28
VSHAPES = [(OB, H), (H,), (H, H), (H,), (H, 1), (1,)]                  # vffc1/w, /b, vffc2/w, /b, vffinal/w, /b
NPI = BN.NP
NVF = sum(int(np.prod(s)) for s in VSHAPES)
HALF_LOG_2PI_E = 0.5 * np.log(2.0 * np.pi * np.e)


def vunflatten(theta):
    out, o = [], 0
    for s in VSHAPES:
        n = int(np.prod(s))
        out.append(np.asarray(theta[o:o + n], dtype=np.float64).reshape(s)); o += n
    return out


def value_forward(theta_vf, mean, std, ob):
    w1, b1, w2, b2, w3, b3 = vunflatten(theta_vf)
    z = np.clip((np.asarray(ob, np.float64) - mean) / std, -5.0, 5.0)
    h1 = np.tanh(z @ w1 + b1)
    h2 = np.tanh(h1 @ w2 + b2)
    return z, h1, h2, (h2 @ w3 + b3)[:, 0]


def neglogp(x, m, ls):
    return 0.5 * (((x - m) / np.exp(ls)) ** 2).sum(-1) + 0.5 * np.log(2.0 * np.pi) * x.shape[-1] + ls.sum(-1)


def lossgrad(theta, mean, std, ob, ac, atarg, old_mean, old_logstd, ret, clip, entcoeff=0.0):
    """theta = [policy (bc_numpy order), value net] -> (losses [6] = pol_surr, pol_entpen, vf_loss, kl, ent, clipfrac; flat gradient)"""
    theta = np.asarray(theta, np.float64)
    tp, tv = theta[:NPI], theta[NPI:]
    w1, b1, w2, b2, w3, b3, ls = BN.unflatten(tp)
    z, h1, h2, m = BN.forward(tp, mean, std, ob)
    x, A = np.asarray(ac, np.float64), np.asarray(atarg, np.float64)
    mo, lo = np.asarray(old_mean, np.float64), np.asarray(old_logstd, np.float64)
    n = x.shape[0]
    ratio = np.exp(neglogp(x, mo, lo) - neglogp(x, m, ls))
    s1, s2 = ratio * A, np.clip(ratio, 1.0 - clip, 1.0 + clip) * A
    first = s1 <= s2
    pol_surr = -np.where(first, s1, s2).mean()
    ent = float((ls + HALF_LOG_2PI_E).sum())
    kl = (ls - lo + (np.exp(2 * lo) + (mo - m) ** 2) / (2.0 * np.exp(2 * ls)) - 0.5).sum(-1).mean()
    clipfrac = float((np.abs(ratio - 1.0) > clip).mean())
    # d pol_surr / d ratio, then through ratio = exp(neglogp_old - neglogp_new)
    c = np.where(first, -A / n, 0.0) * ratio
    inv_var = np.exp(-2.0 * ls)
    G = c[:, None] * (x - m) * inv_var                                 # d / d mean
    gls = (c[:, None] * ((x - m) ** 2 * inv_var - 1.0)).sum(0) - entcoeff
    d2 = (G @ w3.T) * (1.0 - h2 * h2)
    d1 = (d2 @ w2.T) * (1.0 - h1 * h1)
    gp = [z.T @ d1, d1.sum(0), h1.T @ d2, d2.sum(0), h2.T @ G, G.sum(0), gls]
    # value net
    vw1, vb1, vw2, vb2, vw3, vb3 = vunflatten(tv)
    zv, g1, g2, v = value_forward(tv, mean, std, ob)
    e = v - np.asarray(ret, np.float64)
    vf_loss = float((e * e).mean())
    dy = 2.0 * e / n
    e2 = dy[:, None] * vw3[:, 0][None, :] * (1.0 - g2 * g2)
    e1 = (e2 @ vw2.T) * (1.0 - g1 * g1)
    gv = [zv.T @ e1, e1.sum(0), g1.T @ e2, e2.sum(0), g2.T @ dy[:, None], np.array([dy.sum()])]
    losses = np.array([pol_surr, -entcoeff * ent, vf_loss, kl, ent, clipfrac])
    return losses, np.concatenate([t.reshape(-1) for t in gp + gv])


def total_loss(theta, *args, **kw):
    l, _ = lossgrad(theta, *args, **kw)
    return l[0] + l[1] + l[2]
