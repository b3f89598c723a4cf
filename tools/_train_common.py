"""What train_trpo.py, train_ppo.py and train_gail.py share: the env arguments, device / process-group set-up, reading and writing a policy,
and the `--task evaluate` branch."""
import os

import torch

from deepmimic_mujoco_amd import DPVecEnv, MlpPolicy


def add_env_args(ap, reward_help=None, autoreset_help=None, frame_skip_help=None):
    """--motion, --clip-weights, --clip-mode, --obs-mode, --action-mode, --fall-contact, --max-episode-steps, --horizon-termination, --horizon-spd, --bootstrap-time-limit, --log-reward-terms, --perturb and, of --reward, --autoreset and --frame-skip, those whose help text (the scripts' differ) is given."""
    ap.add_argument("--motion", default="walk", help="the clip to imitate, or a comma-separated list (walk,spinkick,kick): one policy on a set of clips, env e on clip e mod K")
    ap.add_argument("--clip-weights", default=None, help="with a list of motions: comma-separated draw probabilities of --clip-mode episode (up to their sum; default uniform)")
    ap.add_argument("--clip-mode", default="fixed", choices=["fixed", "episode"],
                    help="with a list of motions: fixed (default) = an env keeps its clip; episode = every episode start draws the env's clip, as DeepMimic does")
    if reward_help:
        ap.add_argument("--reward", default="alive", help=reward_help)
    ap.add_argument("--obs-mode", default="dp_env_v3", choices=["dp_env_v3", "deepmimic"],
                    help="the observation: dp_env_v3 = the reference's 56 numbers; deepmimic = DeepMimic's 171 state features (phase, root height, every body's "
                         "position / rotation in the root's heading frame and its velocities: one more launch per step).  The policy takes its width from the "
                         "env; at 171 the learners run on their torch paths")
    ap.add_argument("--action-mode", default="raw", choices=["raw", "p-control", "pd", "spd-target", "spd-mocap"],
                    help="what the policy's action is: raw motor commands (default) | p-control, pd: plus a feedback term around the mocap frame | spd-target, spd-mocap: a PD target pose under a stable PD controller evaluated every substep")
    ap.add_argument("--fall-contact", default="none", choices=["none", "deepmimic", "crawl"],
                    help="DeepMimic's early termination: the episode ends when a body of the set touches the floor.  deepmimic = every body except the two ankles; "
                         "crawl = root, chest, neck (the floor clips); none (default) = only the reference's centre-of-mass rule")
    ap.add_argument("--max-episode-steps", type=int, default=0,
                    help="the episode's time limit in env steps (0 = none).  Without --bootstrap-time-limit a time-limit done is a done like any other: the state it cuts off is worth 0")
    ap.add_argument("--horizon-termination", action="store_true",
                    help="run early termination inside the horizon launch (DM_OPT_HORIZON_TERMINATION) instead of a termination launch behind every step launch: "
                         "needs --fall-contact or --max-episode-steps, and an action / observation mode with a horizon launch (not --obs-mode deepmimic; spd-* only with --horizon-spd)")
    ap.add_argument("--horizon-spd", action="store_true",
                    help="--action-mode spd-target / spd-mocap: run the stable PD controller inside the horizon launch (DM_OPT_HORIZON_SPD) instead of one step launch per step; "
                         "not with --obs-mode deepmimic")
    ap.add_argument("--bootstrap-time-limit", action="store_true",
                    help="treat a time-limit end as a truncation (DeepMimic's agent): the value target bootstraps from the critic's value of the state the limit cut off, "
                         "where a fall keeps 0.  Needs --max-episode-steps")
    ap.add_argument("--log-reward-terms", action="store_true",
                    help="--reward imitation: log the reward's five errors (ErrPose, ErrVel, ErrEndEff, ErrRoot, ErrCom) of the states each segment ends in, "
                         "from one more launch per segment")
    ap.add_argument("--perturb", default=None, metavar="bodies=...,force=a:b,duration=a:b,wait=a:b[,z=a:b]",
                    help="DeepMimic's external pushes on a random schedule: a force of a..b newtons on a random body of the set (a set name of --fall-contact, or body names / "
                         "ids joined by +), held for duration a..b env steps, a..b env steps after the last one; z: range of the direction's vertical component "
                         "(default horizontal).  Works with --task evaluate too: a checkpoint's episode length and return under pushes")
    if autoreset_help:
        ap.add_argument("--autoreset", default="init", help=autoreset_help)
    if frame_skip_help:
        ap.add_argument("--frame-skip", default=None, help=frame_skip_help)


def motions(args):
    """--motion as DPVecEnv takes it: a clip name, or the list of a comma-separated value"""
    names = [m for m in str(args.motion).split(",") if m]
    return names if len(names) > 1 else names[0]


def check_env_args(ap, args):
    """Refuse flag combinations that cannot work, with the parser's own error message."""
    many = isinstance(motions(args), list)
    if not many and (getattr(args, "clip_weights", None) or getattr(args, "clip_mode", "fixed") != "fixed"):
        ap.error("--clip-weights and --clip-mode episode need a list of motions: --motion a,b,c")
    if many and getattr(args, "clip_weights", None):
        try:
            w = [float(x) for x in args.clip_weights.split(",")]
        except ValueError:
            ap.error("--clip-weights: comma-separated numbers")
        if len(w) != len(motions(args)):
            ap.error("--clip-weights: one weight per motion (%d), got %d" % (len(motions(args)), len(w)))
    if getattr(args, "bootstrap_time_limit", False) and not args.max_episode_steps > 0:
        ap.error("--bootstrap-time-limit bootstraps the value where the time limit ends an episode: it needs --max-episode-steps M with M > 0")
    if getattr(args, "horizon_spd", False):
        if args.action_mode not in ("spd-target", "spd-mocap"):
            ap.error("--horizon-spd runs the stable PD controller inside the horizon launch: it needs --action-mode spd-target or spd-mocap")
        if args.obs_mode == "deepmimic":
            ap.error("--horizon-spd: --obs-mode deepmimic has no horizon launch")
    if getattr(args, "horizon_termination", False):
        if args.fall_contact == "none" and not args.max_episode_steps > 0:
            ap.error("--horizon-termination runs early termination inside the horizon launch: it needs --fall-contact or --max-episode-steps")
        if (args.action_mode in ("spd-target", "spd-mocap") and not getattr(args, "horizon_spd", False)) or args.obs_mode == "deepmimic":
            ap.error("--horizon-termination: --action-mode spd-* and --obs-mode deepmimic have no horizon launch")
    if getattr(args, "perturb", None):
        from deepmimic_mujoco_amd.perturb import PushSchedule
        try:
            PushSchedule.parse(args.perturb)
        except ValueError as e:
            ap.error("--perturb: %s" % e)
    if getattr(args, "log_reward_terms", False) and getattr(args, "reward", None) != "imitation":
        ap.error("--log-reward-terms takes the imitation reward apart: it needs --reward imitation")


def env_kwargs(args):
    """The DPVecEnv arguments that the env flags set."""
    fs = getattr(args, "frame_skip", None)
    cw = getattr(args, "clip_weights", None)
    return dict(motion=motions(args), clip_weights=[float(x) for x in cw.split(",")] if cw else None, clip_mode=getattr(args, "clip_mode", "fixed"),
                reward=args.reward, action_mode=args.action_mode, obs_mode=args.obs_mode,
                frame_skip=fs if fs in (None, "mocap") else int(fs),
                fall_contact_bodies=None if args.fall_contact == "none" else args.fall_contact, max_episode_steps=args.max_episode_steps,
                horizon_termination=bool(getattr(args, "horizon_termination", False)), horizon_spd=bool(getattr(args, "horizon_spd", False)), perturb=getattr(args, "perturb", None))


def init_device(dist_backend):
    """This rank's GPU and, in a torchrun launch, the process group -> (world, rank, local device index, torch device)."""
    world = int(os.environ.get("WORLD_SIZE", "1")); rank = int(os.environ.get("RANK", "0")); lr = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    if dist_backend == "nccl" and world > ndev:
        raise SystemExit("RCCL needs one GPU per rank: %d ranks, %d devices visible (use --dist-backend gloo to share a GPU)" % (world, ndev))
    lr = lr % max(1, ndev)
    torch.cuda.set_device(lr)
    dev = torch.device("cuda", lr)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)
    return world, rank, lr, dev


def load_policy(path, dev):
    """An .npz (reference variable names) or a tf.train.Saver checkpoint prefix."""
    return MlpPolicy.from_npz(path, device=dev) if path.endswith(".npz") else MlpPolicy.from_tf_checkpoint(path, device=dev)


def save_policy(pi, path):
    """`x.npz`, or a checkpoint prefix -> the tf.train.Saver bundle the reference's `--task evaluate --load_model_path x` restores."""
    if path.endswith(".npz"):
        pi.save_npz(path)
    else:
        pi.save_tf_checkpoint(path)


def eval_setup(args, dev):
    """`--task evaluate` (src/trpo.py:480-487) -> (an env of --number-trajs trajectories, the policy of --load-model-path) for trpo.runner."""
    assert args.load_model_path, "--task %s needs --load-model-path" % args.task
    pi = load_policy(args.load_model_path, dev)
    pi.seed(args.seed)
    return DPVecEnv(args.number_trajs, device=dev.index, autoreset="init", seed=args.seed, **env_kwargs(args)), pi
