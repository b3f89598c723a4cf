#!/usr/bin/env python3
"""Play a motion clip into an animated GIF: the reference's `MocapDM.play` / src/play_mocap.py without a viewer.

Every frame of `data_config` is set as qpos, with the root offset carried from loop to loop as src/mujoco/mocap_v2.py:168-182
does (after each pass the last frame's root x, y are added to the offset), and rendered through the explicit-qpos form of
dm_batch_render — one call per loop, all of its frames at once.

usage: python tools/play_mocap.py --motion walk --camera side --loops 2 --out walk.gif [--width 320 --height 240]
(without PIL the frames go to an .npy next to --out)"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def clip_qpos(cfg, loops):
    """[loops * F, 35]: the clip's frames with the carried root offset of mocap_v2.py:168-182"""
    out, off = [], np.zeros(3)
    for _ in range(int(loops)):
        q = cfg.copy()
        q[:, :3] += off
        out.append(q)
        off = q[-1, :3].copy(); off[2] = 0.0
    return np.concatenate(out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--motion", default="walk", help="a clip name of assets/motions.npz or a DeepMimic motion .txt")
    ap.add_argument("--camera", default="side", choices=["side", "back"])
    ap.add_argument("--loops", type=int, default=2)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="walk.gif")
    args = ap.parse_args(argv)
    from deepmimic_mujoco_amd import Batch
    from deepmimic_mujoco_amd.humanoid import humanoid_spec
    from deepmimic_mujoco_amd.mocap import MocapDM
    from deepmimic_mujoco_amd.model import CompiledModel
    from deepmimic_mujoco_amd.render import FrameWriter
    mc = MocapDM(); mc.load_mocap(args.motion)
    q = clip_qpos(mc.data_config, args.loops)
    b = Batch(CompiledModel(humanoid_spec()), mc.data_config, mc.data_vel, 1, device=args.device, mocap_dt=float(mc.dt))
    frames = b.render(args.width, args.height, args.camera, qpos=q)["rgb"]
    w = FrameWriter(args.out, fps=1.0 / float(mc.dt))
    for f in frames:
        w.add(f)
    path = w.close()
    b.close()
    print("wrote %d frames (%d loops of %s, camera %s, %dx%d) to %s" % (len(frames), args.loops, args.motion, args.camera, args.width, args.height, path))
    return path


if __name__ == "__main__":
    main()
