"""float64 numpy restatement of behaviour cloning (the `behavior_clone.learn` src/gail.py:490-495 calls), written from its formulas:
the policy mean of src/mlp_policy_trpo.py:35-46 (clip included), the loss mean((x - (m + exp(logstd) eps))^2), its flat gradient by
hand-written backpropagation (logstd included), and the device's counter noise normal_from (csrc/rng.h) in numpy uint64 arithmetic with a
float64 Box-Muller.  The tests hold deepmimic_mujoco_amd.behavior_clone (torch path) and the kernels of csrc/pg_kernel.h to it."""
import numpy as np

OB, H, AC = 56, 100, 28
SHAPES = [(OB, H), (H,), (H, H), (H,), (H, AC), (AC,), (AC,)]      # polfc1/w, /b, polfc2/w, /b, polfinal/w, /b, logstd
NP = sum(int(np.prod(s)) for s in SHAPES)
M64 = (1 << 64) - 1


def unflatten(theta):
    out, o = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(np.asarray(theta[o:o + n], dtype=np.float64).reshape(s)); o += n
    return out


def mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def normal_from(seed, counter, idx):
    """h = mix64(mix64(seed ^ counter * 0xD1342543DE82EF95) + idx); u1 = (bits 40..63 + 1) / 2^24, u2 = bits 8..31 / 2^24."""
    with np.errstate(over="ignore"):
        h = mix64(mix64(np.uint64(seed & M64) ^ np.uint64((counter * 0xD1342543DE82EF95) & M64)) + np.asarray(idx, dtype=np.uint64))
    u1 = (((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float64) + 1.0) / 16777216.0
    u2 = ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise(seed, counter, n, stochastic=True):
    """eps [n, 28]: element (s, a) = normal_from(seed, counter, s * 28 + a); zero when not stochastic."""
    if not stochastic:
        return np.zeros((n, AC))
    return normal_from(seed, counter, np.arange(n * AC, dtype=np.uint64)).reshape(n, AC)


def forward(theta, mean, std, ob):
    """-> (z, h1, h2, action mean) in float64; z = clip((ob - mean) / std, +-5)."""
    w1, b1, w2, b2, w3, b3, _ = unflatten(theta)
    z = np.clip((np.asarray(ob, np.float64) - mean) / std, -5.0, 5.0)
    h1 = np.tanh(z @ w1 + b1)
    h2 = np.tanh(h1 @ w2 + b2)
    return z, h1, h2, h2 @ w3 + b3


def loss(theta, mean, std, ob, ac, eps):
    ls = unflatten(theta)[6]
    m = forward(theta, mean, std, ob)[3]
    r = m + np.exp(ls) * eps - np.asarray(ac, np.float64)
    return float((r * r).mean())


def lossgrad(theta, mean, std, ob, ac, eps):
    """-> (loss, flat gradient [NP]) by backpropagation: G = 2 r / (28 n) at the output, d/dlogstd = sum_s G exp(logstd) eps."""
    w1, b1, w2, b2, w3, b3, ls = unflatten(theta)
    z, h1, h2, m = forward(theta, mean, std, ob)
    se = np.exp(ls) * eps
    r = m + se - np.asarray(ac, np.float64)
    n = r.shape[0]
    G = 2.0 * r / (AC * n)
    d2 = (G @ w3.T) * (1.0 - h2 * h2)
    d1 = (d2 @ w2.T) * (1.0 - h1 * h1)
    g = [z.T @ d1, d1.sum(0), h1.T @ d2, d2.sum(0), h2.T @ G, G.sum(0), (G * se).sum(0)]
    return float((r * r).mean()), np.concatenate([x.reshape(-1) for x in g])


def adam_step(theta, m, v, g, t, stepsize=3e-4, beta1=0.9, beta2=0.999, eps=1e-5):
    """MpiAdam.update (src/mpi_adam.py:21-35) in float64: -> (theta, m, v)."""
    a = stepsize * np.sqrt(1 - beta2 ** t) / (1 - beta1 ** t)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    return theta - a * m / (np.sqrt(v) + eps), m, v
