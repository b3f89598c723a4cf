#!/usr/bin/env python3
"""Train the humanoid with the TRPO learner on device-resident rollouts (the reference's `python3 trpo.py`, src/trpo.py:438-491).

    python tools/train_trpo.py --envs 1024 --horizon 64 --seconds 120 [--out gpurun_out/trpo_curve.json]
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 tools/train_trpo.py ...      (one rank per GPU, all-mean'd updates)
"""
import argparse
import json
import os
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only (RCCL across processes)
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _train_common as common  # noqa: E402
from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy  # noqa: E402
from deepmimic_mujoco_amd.trpo import learn  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--vf-batch", type=int, default=4096)
    ap.add_argument("--vf-stepsize", type=float, default=1e-3)
    ap.add_argument("--max-kl", type=float, default=0.01)
    common.add_env_args(ap, reward_help="alive | v3-config | v2-pose | imitation",
                        autoreset_help="init (the reference's trpo.py protocol) | rsi (DeepMimic reference-state initialisation)",
                        frame_skip_help="sim steps per env step, or 'mocap' (default: 1; 'mocap' with --reward imitation)")
    ap.add_argument("--pipeline", type=int, default=2, help="sub-batches whose step launches overlap across consecutive steps (DM_OPT_PIPELINE; with "
                                                            "--unfused: that many env batches on their own streams, policy -> env chains overlap)")
    ap.add_argument("--unfused", action="store_true", help="separate policy launch per step instead of the policy step inside the env step kernel")
    ap.add_argument("--task", default="train", choices=["train", "evaluate"], help="evaluate: the reference's `trpo.py --task evaluate --load_model_path ...`")
    ap.add_argument("--load-model-path", default=None, help="evaluate: a tf.train.Saver checkpoint prefix (the reference's or one written by --save) or an .npz")
    ap.add_argument("--number-trajs", type=int, default=10, help="evaluate: trajectories (one env each; src/trpo.py:483)")
    ap.add_argument("--stochastic-policy", action="store_true")
    ap.add_argument("--save-sample", default=None, help="evaluate: also write the trajectories to this .npz (obs, acs, lens, rets and ep_rets: "
                                                        "the reference's `--save_sample` file, readable by its GAIL expert reader and tools/train_gail.py)")
    ap.add_argument("--render-out", default=None, help="evaluate: write trajectory 0 frame by frame (what the reference's env.render() shows) to this "
                                                       ".gif (an .npy of frames where PIL is missing), ray-cast by dm_batch_render")
    ap.add_argument("--camera", default="side", choices=["side", "back"], help="--render-out: the model camera (dp_env_v3.xml:23-24)")
    ap.add_argument("--width", type=int, default=320, help="--render-out: image width")
    ap.add_argument("--height", type=int, default=240, help="--render-out: image height")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--log-dir", default=None, help="write progress.csv and monitor.csv in the reference's formats")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL, one GPU per rank; gloo = ranks may share a GPU (LOCAL_RANK modulo the visible devices)")
    ap.add_argument("--no-pg-native", action="store_true", help="policy half of the update through torch autograd instead of csrc/pg_kernel.h")
    ap.add_argument("--dump-params", default=None, help="every rank writes its final parameters to <prefix>.rank<r>.npz (replica-consistency checks)")
    ap.add_argument("--save", default=None, help="write the trained policy: `x.npz` (reference variable names) or a checkpoint prefix -> "
                                                 "tf.train.Saver bundle (x.index + x.data-00000-of-00001) the reference's `--task evaluate --load_model_path x` restores")
    args = ap.parse_args()
    common.check_env_args(ap, args)
    world, rank, lr, dev = common.init_device(args.dist_backend)
    kw = common.env_kwargs(args)
    if args.task == "evaluate":                     # src/trpo.py:480-487
        from deepmimic_mujoco_amd.trpo import runner
        env, pi = common.eval_setup(args, dev)
        writer = None
        if args.render_out:
            from deepmimic_mujoco_amd.render import FrameWriter
            writer = FrameWriter(args.render_out, fps=1.0 / (env.frame_skip * float(env._cm.timestep)))
        runner(env, pi, timesteps_per_batch=1024, stochastic_policy=args.stochastic_policy, save_sample=args.save_sample, frames=writer,
               render_size=(args.width, args.height), render_camera=args.camera, reward_terms=args.reward == "imitation")
        if writer is not None:
            print("wrote %d frames of trajectory 0 to %s" % (len(writer.frames), writer.close()))
        return
    P = max(1, args.pipeline)
    if args.unfused:
        cuts = [args.envs * h // P for h in range(P + 1)]
        envs = [DPVecEnv(cuts[h + 1] - cuts[h], device=lr, autoreset=args.autoreset, seed=args.seed + 10000 * rank, env_offset=rank * args.envs + cuts[h], **kw)
                for h in range(P)]
        env = envs if P > 1 else envs[0]
    else:
        from deepmimic_mujoco_amd import _abi as A
        env = DPVecEnv(args.envs, device=lr, autoreset=args.autoreset, seed=args.seed + 10000 * rank, env_offset=rank * args.envs, **kw)
        env.batch.set_option(A.OPT_PIPELINE, min(P, A.MAX_PIPELINE))
    pi = MlpPolicy(ob_dim=(envs[0] if args.unfused else env).observation_space.shape[0], device=dev, seed=args.seed); pi.seed(args.seed + 10000 * rank)
    hist = learn(env, pi, timesteps_per_batch=args.horizon, max_seconds=args.seconds if not args.iters else 0, max_iters=args.iters,
                 vf_batch_size=args.vf_batch, vf_stepsize=args.vf_stepsize, max_kl=args.max_kl, seed=args.seed, log_dir=args.log_dir,
                 fused=False if args.unfused else None, pg_native=False if args.no_pg_native else None, bootstrap_time_limit=args.bootstrap_time_limit,
                 log_reward_terms=args.log_reward_terms)
    if args.dump_params:
        os.makedirs(os.path.dirname(os.path.abspath(args.dump_params)), exist_ok=True)
        pi.save_npz("%s.rank%d.npz" % (args.dump_params, rank))
    if rank == 0:
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            json.dump({"args": vars(args), "world": world, "history": hist}, open(args.out, "w"))
        if args.save:
            common.save_policy(pi, args.save)
        best = max(h["EpLenMeanIter"] for h in hist)
        print("done: %d iterations, %d env steps in %.1f s (%.0f steps/s incl. learner), EpLenMean(last iter) %.1f, best %.1f"
              % (len(hist), hist[-1]["TimestepsSoFar"], hist[-1]["TimeElapsed"], hist[-1]["TimestepsSoFar"] / hist[-1]["TimeElapsed"],
                 hist[-1]["EpLenMeanIter"], best))


if __name__ == "__main__":
    main()
