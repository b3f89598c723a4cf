"""GAE(lambda) with a bootstrap value per row, in float64 numpy, from the formula (include/dmenv.h dm_gae_boot) — not from
the kernel or the torch fallback it checks:

    nonterminal[t] = 1 - new[t+1]                       (new[T] := 0)
    delta[t] = rew[t] + gamma * (vpred[t+1] * nonterminal[t] + vboot[t]) - vpred[t]        (vpred[T] := nextvpred)
    adv[t]   = delta[t] + gamma * lam * nonterminal[t] * adv[t+1]                           (adv[T] := 0)
    tdlamret = adv + vpred

vboot[t] is the value of the state step t left where a time limit truncated the episode there, 0 elsewhere; with vboot = 0 this is
add_vtarg_and_adv of src/trpo.py:83-94 for N environments.  All arrays [T, N] (nextvpred [N]); returns float64."""
import numpy as np


def gae_boot(rew, vpred, new, nextvpred, vboot, gamma, lam):
    rew = np.asarray(rew, dtype=np.float64); vpred = np.asarray(vpred, dtype=np.float64); new = np.asarray(new, dtype=np.float64)
    vboot = np.zeros_like(rew) if vboot is None else np.asarray(vboot, dtype=np.float64)
    T, n = rew.shape
    adv = np.zeros((T, n))
    for e in range(n):                        # one environment at a time, as the reference's single-env loop walks its segment
        carry = 0.0
        for t in range(T - 1, -1, -1):
            ends_here = new[t + 1, e] if t + 1 < T else 0.0
            value_after = vpred[t + 1, e] if t + 1 < T else float(nextvpred[e])
            target = rew[t, e] + gamma * (value_after * (1.0 - ends_here) + vboot[t, e])
            carry = (target - vpred[t, e]) + gamma * lam * (1.0 - ends_here) * carry
            adv[t, e] = carry
    return adv, adv + vpred


def random_segment(T, n, seed, with_vboot=True):
    """A [T, n] segment for the GAE checks: float32 rewards and values, random episode starts, and (with_vboot) bootstrap values where a truncation
    can stand — rows whose successor starts an episode (new[t+1] = 1), and the last row — about half of them non-zero; 0 everywhere else."""
    rng = np.random.RandomState(seed)
    seg = {"rew": rng.randn(T, n).astype(np.float32), "vpred": (3.0 * rng.randn(T, n)).astype(np.float32),
           "new": (rng.rand(T, n) < 0.3).astype(np.int32), "nextvpred": (3.0 * rng.randn(n)).astype(np.float32)}
    if with_vboot:
        may = np.zeros((T, n), dtype=bool)
        may[:-1] = seg["new"][1:] == 1
        may[-1] = True
        seg["vboot"] = np.where(may & (rng.rand(T, n) < 0.5), 3.0 * rng.randn(T, n), 0.0).astype(np.float32)
        seg["vboot"][-1, 0] = 2.5                      # (at least one non-zero entry whatever the draw)
    return seg
