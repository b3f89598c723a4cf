#!/usr/bin/env python3
"""Train the humanoid with PPO (OpenAI baselines' ppo1 `pposgd_simple`, deepmimic_mujoco_amd.ppo) on device-resident rollouts.

    python tools/train_ppo.py --envs 1024 --horizon 64 --seconds 120 [--out ppo_curve.json] [--save ppo-walk]
    python tools/train_trpo.py --task evaluate --load-model-path ppo-walk          (the checkpoint is the reference's format)
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 tools/train_ppo.py ...       (one rank per GPU, all-mean'd gradients)

Defaults are ppo1's run_mujoco: --clip-param 0.2 --entcoeff 0.0 --optim-epochs 10 --optim-stepsize 3e-4 --optim-batchsize 64 --gamma 0.99
--lam 0.95 --adam-epsilon 1e-5; the schedule is linear over --num-timesteps when that is the stopping rule, else constant.
"""
import argparse
import json
import os
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only (RCCL across processes)
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _train_common as common  # noqa: E402
from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy  # noqa: E402
from deepmimic_mujoco_amd.ppo import learn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="train", choices=["train", "evaluate"], help="evaluate: run the policy of --load-model-path (as train_trpo.py does)")
    ap.add_argument("--load-model-path", default=None, help="evaluate: a tf.train.Saver checkpoint prefix or an .npz")
    ap.add_argument("--number-trajs", type=int, default=10, help="evaluate: trajectories (one env each)")
    ap.add_argument("--stochastic-policy", action="store_true")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=64, help="timesteps per env per update (ppo1's timesteps_per_actorbatch / envs)")
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--num-timesteps", type=int, default=0, help="stop after this many env steps (ppo1's max_timesteps; the linear schedule's horizon)")
    ap.add_argument("--clip-param", type=float, default=0.2)
    ap.add_argument("--entcoeff", type=float, default=0.0)
    ap.add_argument("--optim-epochs", type=int, default=10)
    ap.add_argument("--optim-stepsize", type=float, default=3e-4)
    ap.add_argument("--optim-batchsize", type=int, default=64, help="0: the whole batch")
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--adam-epsilon", type=float, default=1e-5)
    ap.add_argument("--schedule", default=None, choices=["constant", "linear"], help="default: linear with --num-timesteps, else constant")
    ap.add_argument("--no-native", action="store_true", help="the update through torch autograd instead of the dm_ppo_* kernels")
    common.add_env_args(ap, reward_help="alive | v3-config | v2-pose | imitation",
                        autoreset_help="init (the reference's protocol) | rsi (DeepMimic reference-state initialisation)",
                        frame_skip_help="sim steps per env step, or 'mocap' (default: 1)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="write the per-iteration statistics as JSON")
    ap.add_argument("--log-dir", default=None, help="write progress.csv and monitor.csv in the reference's formats")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"])
    ap.add_argument("--save", default=None, help="write the trained policy: `x.npz` or a checkpoint prefix (the tf.train.Saver bundle the "
                                                 "reference's `--task evaluate --load_model_path x` restores)")
    args = ap.parse_args()
    common.check_env_args(ap, args)
    world, rank, lr, dev = common.init_device(args.dist_backend)
    if args.task == "evaluate":
        from deepmimic_mujoco_amd.trpo import runner
        env, pi = common.eval_setup(args, dev)
        runner(env, pi, timesteps_per_batch=1024, stochastic_policy=args.stochastic_policy)
        return
    env = DPVecEnv(args.envs, device=lr, autoreset=args.autoreset, seed=args.seed + 10000 * rank, env_offset=rank * args.envs, **common.env_kwargs(args))
    pi = MlpPolicy(ob_dim=env.observation_space.shape[0], device=dev, seed=args.seed); pi.seed(args.seed + 10000 * rank)
    stop = dict(max_iters=args.iters) if args.iters else dict(max_timesteps=args.num_timesteps) if args.num_timesteps else dict(max_seconds=args.seconds)
    schedule = args.schedule or ("linear" if "max_timesteps" in stop else "constant")
    hist = learn(env, pi, timesteps_per_batch=args.horizon, clip_param=args.clip_param, entcoeff=args.entcoeff, optim_epochs=args.optim_epochs,
                 optim_stepsize=args.optim_stepsize, optim_batchsize=args.optim_batchsize or None, gamma=args.gamma, lam=args.lam,
                 adam_epsilon=args.adam_epsilon, schedule=schedule, seed=args.seed, log_dir=args.log_dir, native=False if args.no_native else None, bootstrap_time_limit=args.bootstrap_time_limit,
                 log_reward_terms=args.log_reward_terms, **stop)
    if rank == 0:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump({"args": vars(args), "world": world, "history": hist}, open(args.out, "w"))
        if args.save:
            common.save_policy(pi, args.save)
        if hist:
            h = hist[-1]
            print("done: %d iterations, %d env steps in %.1f s, EpLenMean %.1f (last iter %.1f), loss_kl %.5f, clipfrac %.3f"
                  % (len(hist), h["TimestepsSoFar"], h["TimeElapsed"], h["EpLenMean"], h["EpLenMeanIter"], h["loss_kl"], h["clipfrac"]))


if __name__ == "__main__":
    main()
