"""DeepMimic's state features as an observation (`obs_mode="deepmimic"`): the layout of a feature row and the phase rule.

Specification: `cCtController::BuildStatePose` / `BuildStateVel` as quoted in the reference's porting notes (`code.md:307-489`) —
the reference itself never built it: every one of its environments returns `dp_env_v3`'s 56 numbers (hinge angles and hinge
rates), which carry neither the root's height or orientation, nor the bodies' positions, nor the position in the clip.  The values
are computed on the device by `dm_batch_state_features` (`csrc/state_features.h`, `csrc/state_kernel.h`; `Batch.state_features`);
nothing here computes them.  Layout of a row (NSTATE = 171 doubles = 1 + 1 + 13 * 7 + 13 * 6); coordinates are the MuJoCo
model's (z up, x forward); bodies are model bodies b = 1..13 in model order (root, chest, neck, right_shoulder, right_elbow,
left_shoulder, left_elbow, right_hip, right_knee, right_ankle, left_hip, left_knee, left_ankle), k = b - 1:

    0                     phase in [0, 1)
    1                     root height: z of the root body's frame origin (xpos[1][2])
    2 + 7k .. +3          Rz(-hd) (xipos_b - xpos_root): the body's centre of mass relative to the root's frame origin, in the heading
                          frame (the root's own entry is its centre-of-mass offset, not a special case)
    2 + 7k + 3 .. +4      q_z(-hd) (x) xquat_b as (w, x, y, z), negated as a whole when w < 0             (code.md:406-412)
    93 + 6k .. +3         Rz(-hd) v_b, v_b the world velocity of the point xipos_b
    93 + 6k + 3 .. +3     Rz(-hd) w_b, w_b the body's world angular velocity

Heading: hd = atan2(f_y, f_x), f the root's x axis in the world, the root quaternion normalised first — `imitation.py`'s heading
(the end-effector features of the reward).  qvel[0:3] is the world velocity of the root's frame origin; qvel[3:6] is the root's
angular velocity in its own frame (MuJoCo's free joint, as in `imitation.ImitationSpec.features`).  Upstream's defaults otherwise:
no `flip_stance`; `mRecordWorldRootPos` / `mRecordWorldRootRot` off.  The sign rule makes the quaternion discontinuous where its w
crosses 0.

Phase (`phase_of`): the batch's frame cursor over the clip's length.  Reward modes "alive", "v3-config" and "imitation" keep the
cursor in `frame_idx` ("alive" never advances it: the phase stays the RSI draw); "v2-pose" and "v1-quat" count steps from 0 in
`frame_idx` and add the RSI draw `frame_init`.  For "v1-quat" that is the STEP cursor: it is the mocap frame only when one env step
spans one mocap frame.
"""
import numpy as np

from ._abi import NSTATE

NBODY = 13
POSE_W, VEL_W = 7, 6
O_PHASE, O_HEIGHT, O_POS, O_VEL = 0, 1, 2, 2 + POSE_W * NBODY
assert O_VEL == 93 and O_VEL + VEL_W * NBODY == NSTATE == 171

# Observation by name.  "dp_env_v3": the reference's 56 numbers (hinge angles, hinge rates), written by the step launch itself.  "deepmimic": the 171 state
# features above, computed by one more launch on the same stream after the step from the state the step left — the fresh episode's after an auto-reset.
OBS_MODES = ("dp_env_v3", "deepmimic")


def obs_width(obs_mode):
    """Width of an observation row: 56 for "dp_env_v3" (the default), NSTATE for "deepmimic"; anything else raises ValueError."""
    if obs_mode not in OBS_MODES:
        raise ValueError("obs_mode must be one of %s" % (OBS_MODES,))
    return NSTATE if obs_mode == "deepmimic" else 56


def phase_of(reward_mode, frame_idx, frame_init, n_frames):
    """Phase in [0, 1) of the clip from a batch's cursor fields (ints, integer arrays or torch tensors); reward_mode: 0..4 or a name of
    `dp_env.REWARD_MODES`."""
    if isinstance(reward_mode, str):
        from .dp_env import REWARD_MODES
        reward_mode = REWARD_MODES[reward_mode]
    if type(frame_idx).__module__.startswith("torch"):      # tensors stay tensors, on their device (float64 like the numpy form)
        import torch
        k = frame_idx.to(torch.int64)
        if int(reward_mode) in (2, 4):
            k = k + torch.as_tensor(frame_init, device=k.device).to(torch.int64)
        return (k % int(n_frames)).to(torch.float64) / float(n_frames)
    k = np.asarray(frame_idx, dtype=np.int64)
    if int(reward_mode) in (2, 4):
        k = k + np.asarray(frame_init, dtype=np.int64)
    return (k % int(n_frames)) / float(n_frames)
