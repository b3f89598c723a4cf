#!/usr/bin/env python3
"""Generate tests/golden/gail_ref_golden.npz by EXECUTING the reference's GAIL helpers on small seeded inputs.

Follows make_learner_fixture.py's rules: runs only where the reference tree is (REF below); nothing of it is copied into the repo — its
modules are imported from where they lie, or the ONE function under test is cut out of the module's syntax tree in memory — and only
input / output DATA is written.

  imported as it is (numpy only):
    Dset / Mujoco_Dset            src/utils/mujoco_dset.py       batch sequences of get_next_batch after np.random.seed(s), on a dense
                                                                 (N, L, dim) file and on a ragged one (object arrays); batches larger than
                                                                 the dataset included.  Stand-in: the module's `np.load` is given
                                                                 allow_pickle=True (numpy >= 1.16.3 refuses object arrays otherwise)
  executed from the syntax tree (src/gail.py imports tensorflow / mpi4py / gym):
    traj_segment_generator        src/gail.py:27-92              rew / ep_rets / ep_true_rets / ep_lens of consecutive segments, against the
                                                                 stand-in env / policy / reward_giver below; every env step's (ob, ac,
                                                                 true reward, done) is recorded so the repo's collector can be fed the same

What the repo's code (deepmimic_mujoco_amd/gail.py ExpertDataset, rollout.SegmentCollector's reward_giver hook) is held to: tests/test_gail.py.
"""
import ast
import importlib.util
import os
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
REF = "/root/reference/src"
OUT = os.path.join(REPO, "tests", "golden", "gail_ref_golden.npz")


def cut(path, name, kind):
    tree = ast.parse(open(path).read())
    for node in tree.body:
        if isinstance(node, kind) and node.name == name:
            return compile(ast.Module(body=[node], type_ignores=[]), path, "exec")
    raise KeyError(name)


def _row_data(n_traj, lens, seed):
    """obs[..., 0] / acs[..., 0] = the global transition index: a batch names its rows"""
    rng = np.random.RandomState(seed)
    obs, acs, k = [], [], 0
    for L in lens:
        o = rng.randn(L, 56); a = rng.randn(L, 28).astype(np.float32)
        o[:, 0] = np.arange(k, k + L); a[:, 0] = np.arange(k, k + L)
        obs.append(o); acs.append(a); k += L
    return obs, acs


# ---- stand-ins for the generator ---------------------------------------------------------------------------------------------
class Space(object):
    def __init__(self, n):
        self.n = n

    def sample(self):
        return np.zeros(self.n, dtype=np.float32)


class StandInEnv(object):
    """deterministic: episode k lasts 3 + (7 k) % 11 steps; true reward 0.1 t + 0.01 k; obs a smooth function of (k, t)"""
    action_space = Space(28)

    def __init__(self):
        self.k, self.t, self.log = -1, 0, []

    def _ob(self):
        return np.sin(0.3 * np.arange(56) + 0.7 * self.k + 0.11 * self.t)

    def reset(self):
        self.k += 1; self.t = 0
        self.cur = self._ob()
        return self.cur

    def step(self, ac):
        ob_before = self.cur
        self.t += 1
        rew = 0.1 * self.t + 0.01 * self.k
        done = self.t >= 3 + (7 * self.k) % 11
        self.cur = self._ob()
        self.log.append((ob_before, np.asarray(ac, dtype=np.float32).copy(), rew, done))
        return self.cur, rew, done, {}


class StandInPi(object):
    def act(self, stochastic, ob):
        return np.tanh(0.5 * ob[:28]).astype(np.float32), np.float32(ob.sum() * 0.1)


def standin_reward(ob, ac):
    """the stand-in discriminator's reward, float32 like the reference's graph; tests/test_gail.py restates it"""
    return np.float32(0.3 * np.sin(np.sum(ob) * 0.5) + 0.05 * np.sum(ac) + 1.0)


class StandInD(object):
    def get_reward(self, ob, ac):
        return np.array([[standin_reward(ob, ac)]], dtype=np.float32)


def main():
    out = {}
    # ---- Dset / Mujoco_Dset ------------------------------------------------------------------------------------------------------
    spec = importlib.util.spec_from_file_location("ref_mujoco_dset", os.path.join(REF, "utils", "mujoco_dset.py"))
    md = importlib.util.module_from_spec(spec); spec.loader.exec_module(md)
    shim = types.SimpleNamespace(**{k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    shim.load = lambda p, **kw: np.load(p, allow_pickle=True)
    md.np = shim
    tmp = tempfile.mkdtemp()
    cases = {"dense": ([6] * 4, "ep_rets"), "ragged": ([4, 7, 2, 5], "ep_rets")}
    sizes = [3, 5, 4, 7, 30, 2, 6, 1, 9]                          # 30 > every dataset here: the short batch
    for name, (lens, key) in cases.items():
        obs, acs = _row_data(len(lens), lens, seed=len(name))
        if name == "dense":
            O, A = np.stack(obs), np.stack(acs)
        else:
            O = np.empty(len(lens), dtype=object); A = np.empty(len(lens), dtype=object)
            for i in range(len(lens)):
                O[i] = obs[i]; A[i] = acs[i]
        rets = np.array([float(L) * 1.5 for L in lens])
        path = os.path.join(tmp, name + ".npz")
        np.savez(path, obs=O, acs=A, lens=np.array(lens), **{key: rets})
        out[name + "_obs"] = np.concatenate(obs); out[name + "_acs"] = np.concatenate(acs); out[name + "_lens"] = np.array(lens)
        out[name + "_rets"] = rets
        for seed, tl in ((3, -1), (11, 2)):
            np.random.seed(seed)
            d = md.Mujoco_Dset(expert_path=path, traj_limitation=tl)
            seq = [d.get_next_batch(b)[0][:, 0].astype(np.int64) for b in sizes]
            tag = "%s_s%d_tl%d" % (name, seed, tl)
            out[tag + "_batch_lens"] = np.array([len(s) for s in seq])
            out[tag + "_batch_rows"] = np.concatenate(seq)
            out[tag + "_meta"] = np.array([d.num_traj, d.num_transition, d.avg_ret, d.std_ret])
    out["dset_sizes"] = np.array(sizes)

    # ---- gail.traj_segment_generator ------------------------------------------------------------------------------------------
    ns = {"np": np}
    exec(cut(os.path.join(REF, "gail.py"), "traj_segment_generator", ast.FunctionDef), ns)
    env, pi, T, K = StandInEnv(), StandInPi(), 16, 5
    gen = ns["traj_segment_generator"](pi, env, StandInD(), T, True)
    rew, rets, true_rets, lens, counts = [], [], [], [], []
    for _ in range(K):
        seg = gen.__next__()
        rew.append(np.array(seg["rew"], dtype=np.float32))
        rets += [float(np.asarray(r).reshape(())) for r in seg["ep_rets"]]
        true_rets += [float(r) for r in seg["ep_true_rets"]]
        lens += [int(x) for x in seg["ep_lens"]]
        counts.append(len(seg["ep_lens"]))
    steps = K * T
    out["gen_T"] = np.array([T, K])
    out["gen_ob"] = np.stack([x[0] for x in env.log[:steps]])          # step t: the observation acted on, the action, the env's reward, done
    out["gen_ac"] = np.stack([x[1] for x in env.log[:steps]])
    out["gen_true_rew"] = np.array([x[2] for x in env.log[:steps]])
    out["gen_done"] = np.array([x[3] for x in env.log[:steps]], dtype=np.uint8)
    out["gen_rew"] = np.stack(rew)
    out["gen_ep_rets"], out["gen_ep_true_rets"], out["gen_ep_lens"] = np.array(rets), np.array(true_rets), np.array(lens)
    out["gen_ep_counts"] = np.array(counts)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, sorted(out))


if __name__ == "__main__":
    main()
