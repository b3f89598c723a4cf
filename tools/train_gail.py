#!/usr/bin/env python3
"""Train the humanoid with GAIL on device-resident rollouts (the reference's `python3 gail.py`, src/gail.py:420-493).

    python tools/train_trpo.py --task evaluate --load-model-path tests/golden/ckpt/trpo-walk-0 --save-sample expert.npz
    python tools/train_gail.py --expert-path expert.npz --envs 4096 --horizon 128 --seconds 120 [--save gail.npz]
    python tools/train_gail.py --expert-path expert.npz --pretrained --BC-max-iter 2000 --bc-save bc ...   (GAIL from a behaviour-cloned policy)

--task evaluate runs the policy of --load-model-path like train_trpo.py's; --task sample does the same and writes the trajectories
(--save-sample, default sample.npz).  --save writes the policy as train_trpo.py --save does and the adversary's variables to
<save without .npz>.adversary.npz.
--pretrained clones the expert first (src/gail.py:490-495, behavior_clone.learn: --BC-max-iter Adam iterations of 128 transitions) and GAIL
starts from that policy; --bc-save writes the cloned policy (x.npz or a checkpoint prefix) for train_trpo.py --task evaluate.
--algo ppo updates the policy with PPO (deepmimic_mujoco_amd.ppo) instead of TRPO.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _train_common as common  # noqa: E402
from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy  # noqa: E402
from deepmimic_mujoco_amd import behavior_clone  # noqa: E402
from deepmimic_mujoco_amd.gail import ExpertDataset, TransitionClassifier, learn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--expert-path", default=None, help="expert trajectories: an .npz with obs / acs and ep_rets or rets")
    ap.add_argument("--traj-limitation", type=int, default=-1)
    ap.add_argument("--g-step", type=int, default=3, help="policy updates per iteration")
    ap.add_argument("--d-step", type=int, default=1, help="discriminator minibatches per iteration")
    ap.add_argument("--adversary-hidden-size", type=int, default=100)
    ap.add_argument("--adversary-entcoeff", type=float, default=1e-3)
    ap.add_argument("--policy-entcoeff", type=float, default=0.0)
    ap.add_argument("--d-stepsize", type=float, default=3e-4)
    ap.add_argument("--max-kl", type=float, default=0.01)
    ap.add_argument("--algo", default="trpo", choices=["trpo", "ppo"], help="the policy's learner (the reference's --algo); ppo: ppo1's defaults")
    ap.add_argument("--task", default="train", choices=["train", "evaluate", "sample"])
    ap.add_argument("--load-model-path", default=None, help="evaluate / sample: a tf.train.Saver checkpoint prefix or an .npz")
    ap.add_argument("--number-trajs", type=int, default=10)
    ap.add_argument("--stochastic-policy", action="store_true")
    ap.add_argument("--save-sample", default=None)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=1024, help="timesteps_per_batch (src/gail.py:472)")
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--num-timesteps", type=int, default=0, help="stop after this many timesteps of finished episodes (the reference's --num_timesteps)")
    common.add_env_args(ap)
    ap.add_argument("--reward", default="alive", help="the env's own reward (logged as EpTrueRewMean)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the per-iteration statistics as JSON")
    ap.add_argument("--log-dir", default=None, help="write progress.csv and monitor.csv in the reference's formats")
    ap.add_argument("--save", default=None, help="write the trained policy (x.npz or a checkpoint prefix) and the adversary (x.adversary.npz)")
    ap.add_argument("--pretrained", action="store_true", help="behaviour-clone the expert before GAIL (the reference's --pretrained)")
    ap.add_argument("--BC-max-iter", dest="BC_max_iter", type=int, default=10000, help="--pretrained: BC iterations (the reference's --BC_max_iter)")
    ap.add_argument("--bc-save", default=None, help="--pretrained: write the cloned policy (x.npz or a checkpoint prefix) before GAIL")
    args = ap.parse_args()
    common.check_env_args(ap, args)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.task in ("evaluate", "sample"):
        from deepmimic_mujoco_amd.trpo import runner
        env, pi = common.eval_setup(args, dev)
        save = args.save_sample or ("sample.npz" if args.task == "sample" else None)
        runner(env, pi, timesteps_per_batch=1024, stochastic_policy=args.stochastic_policy, save_sample=save)
        return
    assert args.expert_path, "--task train needs --expert-path"
    expert = ExpertDataset(args.expert_path, traj_limitation=args.traj_limitation, seed=args.seed, device=dev)
    env = DPVecEnv(args.envs, device=0, autoreset="init", seed=args.seed, **common.env_kwargs(args))
    pi = MlpPolicy(ob_dim=env.observation_space.shape[0], device=dev, seed=args.seed); pi.seed(args.seed)
    if args.pretrained:                                     # src/gail.py:490-495
        t0 = time.time()
        train, _ = behavior_clone.learn(pi, expert, max_iters=args.BC_max_iter, verbose=True, seed=args.seed)
        print("BC done: %d iterations in %.2f s, train loss %.6f -> %.6f (mean of the first / last %d)"
              % (len(train), time.time() - t0, train[:100].mean(), train[-100:].mean(), min(100, len(train))))
        if args.bc_save:
            common.save_policy(pi, args.bc_save)
    reward_giver = TransitionClassifier(ob_dim=env.observation_space.shape[0], hidden_size=args.adversary_hidden_size, entcoeff=args.adversary_entcoeff, device=dev, seed=args.seed)
    stop = dict(max_iters=args.iters) if args.iters else dict(max_timesteps=args.num_timesteps) if args.num_timesteps else dict(max_seconds=args.seconds)
    hist = learn(env, pi, reward_giver, expert, g_step=args.g_step, d_step=args.d_step, d_stepsize=args.d_stepsize, timesteps_per_batch=args.horizon,
                 entcoeff=args.policy_entcoeff, max_kl=args.max_kl, seed=args.seed, log_dir=args.log_dir, algo=args.algo, bootstrap_time_limit=args.bootstrap_time_limit,
                 log_reward_terms=args.log_reward_terms, **stop)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({"args": vars(args), "history": hist}, open(args.out, "w"))
    if args.save:
        common.save_policy(pi, args.save)
        reward_giver.save_npz((args.save[:-4] if args.save.endswith(".npz") else args.save) + ".adversary.npz")
    if hist:
        h = hist[-1]
        print("done: %d iterations in %.1f s, EpLenMean %.1f, EpRewMean %.3f, EpTrueRewMean %.3f, generator_acc %.3f, expert_acc %.3f"
              % (len(hist), h["TimeElapsed"], h["EpLenMean"], h["EpRewMean"], h["EpTrueRewMean"], h["generator_acc"], h["expert_acc"]))


if __name__ == "__main__":
    main()
