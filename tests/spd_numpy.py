"""float64 restatement of action modes 3 ("spd-target") and 4 ("spd-mocap") on the CPU oracle (TEST INFRASTRUCTURE).

The stable PD rule (cImpPDController::CalcControlForces, code.md:147-179), evaluated at the start of every simulation substep from the
state (q, v) that substep starts at, h = the model's timestep:

    p = kp (qbar - q - h v)        d = kd (vbar - v)         (dofs 6..33; 0 on the root dofs)
    c = qfrc_bias - qfrc_passive
    a = (M + h diag(kd))^-1 (p + d - c)                      (dense solve on the full 34 x 34 matrix)
    tau = p + d - h kd a           ctrl_u = tau_{6+u} / gear_u   (unclamped in data.ctrl; the oracle's step clamps to ctrlrange)

Nothing here is taken from the code under test: M, qfrc_bias, qfrc_passive come from the oracle's forward(), the solve is numpy's."""
import math

import numpy as np

from deepmimic_mujoco_amd.mocap import PARAMS_KP_KD


def gains(cm):
    """(kp, kd) per dof [34]; zero on the six root dofs."""
    kp = np.zeros(cm.nv); kd = np.zeros(cm.nv)
    for d in range(6, cm.nv):
        kp[d], kd[d] = PARAMS_KP_KD[cm.body_names[cm.dof_bodyid[d]]]
    return kp, kd


def targets(mode, action, mc, frame_idx):
    """(qbar, vbar) [28] of one env from its action and the frame cursor at the start of the env step."""
    a = np.asarray(action, dtype=np.float64)
    if mode == 3:
        return a.copy(), np.zeros(28)
    assert mode == 4
    return mc.data_config[frame_idx][7:] + a, mc.data_vel[frame_idx][6:].copy()


def smooth_terms(od):
    """forward() at the data's state without disturbing the warm start: (M [34, 34], c = qfrc_bias - qfrc_passive, qpos, qvel)."""
    ws = od.get("qacc_warmstart").copy()
    od.forward()
    od.set("qacc_warmstart", ws)
    M = od.get("M").reshape(34, 34).copy()
    c = od.get("qfrc_bias") - od.get("qfrc_passive")
    return M, c, od.get("qpos").copy(), od.get("qvel").copy()


def spd_ctrl(cm, od, qbar, vbar, h):
    """the unclamped ctrl [28] of the rule above at the oracle data's current state"""
    kp, kd = gains(cm)
    M, c, q, v = smooth_terms(od)
    p = np.zeros(34); d = np.zeros(34)
    p[6:] = kp[6:] * (qbar - q[7:] - h * v[6:])
    d[6:] = kd[6:] * (vbar - v[6:])
    a = np.linalg.solve(M + h * np.diag(kd), p + d - c)
    tau = p + d - h * kd * a
    return tau[6:] / cm.actuator_gear


def substep(cm, od, qbar, vbar, h):
    """one simulation substep under the controller; returns the ctrl it applied"""
    ctrl = spd_ctrl(cm, od, qbar, vbar, h)
    od.set("ctrl", ctrl)
    od.step()
    return ctrl


def update_interval(mocap_dt, h, n_substeps):
    """dp_env_v1's update interval (reward mode 4): env steps per mocap frame, int(mocap_dt // dt), at least 1"""
    return max(1, int(math.floor(mocap_dt / (h * n_substeps))))


def start_frame(reward_mode, cursor, frame_init, n_frames, upd=1):
    """The mocap frame an env is at as the env step starts (include/dmenv.h DM_OPT_ACTION_MODE): the cursor itself in reward modes 0, 1 and 3; in
    modes 2 and 4 the cursor counts steps and the draw is added at look-up (src/dp_env_v2.py:128-129, src/dp_env_v1.py:94-96)."""
    if reward_mode == 2:
        return (cursor + frame_init) % n_frames
    if reward_mode == 4:
        return (cursor // upd + frame_init) % n_frames
    return cursor


def env_step(cm, od, mode, action, mc, frame_idx, n_substeps, h, reward_mode=0, frame_init=0, imit=None, cycle=0, peak=None):
    """DPEnv.step of one oracle env in action mode 3 / 4: (obs, reward, done, next frame cursor, last substep's unclamped ctrl).
    `frame_idx` is the env's cursor, `frame_init` its drawn frame; mode 4 tracks start_frame() of the two.  The reward is the oracle's own epilogue
    on the state the substeps leave: reward modes 0 (alive), 1 (v3-config), 2 (v2-pose) through a zero-substep Data.env_step, 3 (imitation;
    imit = (table, params); the cursor returned is the pair (cursor, cycle)) through a zero-substep env_step_imitation, 4 (v1-quat) restated
    from dmo_env_step_v1 on the oracle's feature and reward routines (its interval divides by the substep count, so zero substeps cannot be
    asked of it).  Reward modes 2 and 4 charge the LAST substep's unclamped ctrl — what data.ctrl holds when the reference reads it.
    peak: a one-element list that collects the largest constraint row count of the substeps' evaluations."""
    from oracle import oracle as O
    F = mc.data_config.shape[0]
    upd = update_interval(float(mc.dt), h, n_substeps) if reward_mode == 4 else 1
    qbar, vbar = targets(mode, action, mc, start_frame(reward_mode, frame_idx, frame_init, F, upd))
    ctrl = None
    for _ in range(n_substeps):
        ctrl = substep(cm, od, qbar, vbar, h)
        if peak is not None:
            peak[0] = max(peak[0], int(od.get("nefc_peak", 1)[0]))
    if reward_mode in (0, 1, 2):
        obs, rew, done, nxt = od.env_step(ctrl, 0, reward_mode, mc.data_config, frame_idx, frame_init)
    elif reward_mode == 3:
        obs, rew, done, nxt, cycle = O.env_step_imitation(od.m, od, ctrl, 0, imit[0], imit[1], frame_idx, cycle)
        nxt = (nxt, cycle)
    else:
        assert reward_mode == 4
        obs, done, nxt = od.obs(), od.is_done(), frame_idx + 1
        rew = 0.0
        if nxt % upd == 0:
            k = (nxt // upd + frame_init) % F
            f0 = O.imitation_features(od.m, od.get("qpos", 40), od.get("qvel", 40), imit[1])
            rew = O.v1_reward(od.m, f0, imit[0][k], imit[0][min(k + 1, F - 1)], imit[1])[0]
        rew -= 0.1 * float(np.square(ctrl).sum())
    return obs, rew, done, nxt, ctrl
