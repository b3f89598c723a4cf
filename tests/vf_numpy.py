"""float64 numpy restatement of ONE epoch of the value fit (src/trpo.py:288-295) as dm_vf_fit_epoch runs it — TEST INFRASTRUCTURE.

Per minibatch, in order: `Rms.update` (tests/trpo_numpy.py); the float32 mean and std the filter publishes — float32(sum / count),
float32(sumsq / count) - mean^2 floored at 1e-2, then the square root; normalise and clip to +-5; `vf_forward` / `vf_backward` with
dy = 2 (v - ret) / bs; the MpiAdam rule (src/mpi_adam.py:21-35) with the step scales the caller passes.  Everything but the published mean / std
is float64.  `dtype=np.float32` runs the network and Adam in float32 instead: the rounding envelope a float32 implementation of the same
formulas has against this one (the filter's sums stay float64, as on the device)."""
import numpy as np

from tests import ppo_numpy as PN
from tests import trpo_numpy as TN

VF = TN.VF
SHAPES = dict(zip(VF, PN.VSHAPES))                                     # one statement of the value net's shapes: tests/ppo_numpy.py
NP = sum(int(np.prod(s)) for s in SHAPES.values())


def unflat(theta, dtype=np.float64):
    out, o = {}, 0
    for k in VF:
        n = int(np.prod(SHAPES[k]))
        out[k] = np.asarray(theta[o:o + n], dtype=dtype).reshape(SHAPES[k]); o += n
    return out


def published(rms):
    """the filter's float32 mean and std (RunningMeanStd._refresh of deepmimic_mujoco_amd/policy.py, k_vf_rms of csrc/vf_kernel.h)"""
    m = (rms.sum / rms.count).astype(np.float32)
    var = (rms.sumsq / rms.count).astype(np.float32) - m * m
    return m, np.sqrt(np.maximum(var, np.float32(1e-2)))


def normalise(ob, mean32, std32, dtype=np.float64):
    return np.clip((np.asarray(ob, dtype) - mean32.astype(dtype)) / std32.astype(dtype), -5.0, 5.0)


def loss(theta, z, ret):
    v, _ = TN.vf_forward(unflat(theta), z)
    return float(((v - ret) ** 2).mean())


def gradient(theta, z, ret, dtype=np.float64):
    """-> flat gradient of mean((v(z) - ret)^2), in `dtype` arithmetic"""
    p = unflat(theta, dtype)
    v, cache = TN.vf_forward(p, np.asarray(z, dtype))
    dy = (dtype(2.0) * (v - np.asarray(ret, dtype)) / dtype(len(ret))).astype(dtype)
    if dtype is np.float64:
        return TN.vf_backward(p, cache, dy)
    x, h1, h2 = cache
    dv = dy[:, None]
    g = {"vffinal/w": h2.T @ dv, "vffinal/b": dv.sum(0)}
    dz2 = (dv @ p["vffinal/w"].T) * (1 - h2 * h2)                       # TN.vf_backward, without its conversion to float64
    g["vffc2/w"] = h1.T @ dz2; g["vffc2/b"] = dz2.sum(0)
    dz1 = (dz2 @ p["vffc2/w"].T) * (1 - h1 * h1)
    g["vffc1/w"] = x.T @ dz1; g["vffc1/b"] = dz1.sum(0)
    return np.concatenate([g[k].reshape(-1) for k in VF])


def fit_epoch(theta, m, v, rms, ob, ret, nb, bs, scales, beta1, beta2, eps, dtype=np.float64):
    """One epoch of `nb` minibatches of `bs` rows of ob [nb * bs, 56] / ret [nb * bs].  `rms`: a TN.Rms, updated in place (the filter state
    after the epoch).  -> a list with one dict per minibatch: g, m, v, theta after it, the published mean / std it normalised with, and z."""
    theta, m, v = (np.array(a, dtype=dtype) for a in (theta, m, v))
    b1, b2, e = dtype(beta1), dtype(beta2), dtype(eps)
    out = []
    for i in range(nb):
        x, r = ob[i * bs:(i + 1) * bs], ret[i * bs:(i + 1) * bs]
        rms.update(x)
        mean32, std32 = published(rms)
        z = normalise(x, mean32, std32, dtype)
        g = gradient(theta, z, r, dtype)
        m = b1 * m + (dtype(1.0) - b1) * g
        v = b2 * v + (dtype(1.0) - b2) * g * g
        theta = theta - dtype(scales[i]) * m / (np.sqrt(v) + e)
        out.append(dict(g=g, m=m.copy(), v=v.copy(), theta=theta.copy(), mean=mean32, std=std32, z=z))
    return out
