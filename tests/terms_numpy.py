"""Float64 restatement of the imitation reward's terms row (include/dmenv.h DM_NTERMS = 28; deepmimic_mujoco_amd/imitation.py has the
column offsets): from `ImitationSpec.features` of the state, one row of the reference table and the formulas of the contract, written
out term by term so that the joint shares and the end-effector distances exist on their own."""
import numpy as np

from deepmimic_mujoco_amd.imitation import (NEE, NJ, O_COMV, O_EE, O_JQ, O_JW, O_RANG, O_RLIN, O_RPOS, O_RQUAT, TERM_SCALE, TERM_W,
                                            quat_diff_theta)

NTERMS = 28
O_ERR, O_TERM, O_SUM, O_JOINT, O_ENDEFF = 0, 5, 10, 11, 24


def row_from_features(spec, f0, f1, root_shift=(0.0, 0.0)):
    """the 28 numbers of simulated features f0 against reference features f1 whose root has advanced by root_shift"""
    row = np.zeros(NTERMS)
    th_root = quat_diff_theta(f0[O_RQUAT:O_RQUAT + 4], f1[O_RQUAT:O_RQUAT + 4])
    dw_root = f1[O_RANG:O_RANG + 3] - f0[O_RANG:O_RANG + 3]
    vel = spec.w_root * dw_root.dot(dw_root)
    row[O_JOINT + NJ] = spec.w_root * th_root ** 2                      # the root is weight slot 12
    for g, b in enumerate(spec.bodies):
        q0, q1 = f0[O_JQ + 4 * g:O_JQ + 4 * g + 4], f1[O_JQ + 4 * g:O_JQ + 4 * g + 4]
        th = (q1[0] - q0[0]) if spec.cm.body_dofnum[b] == 1 else quat_diff_theta(q0, q1)
        row[O_JOINT + g] = spec.w_joint[g] * th ** 2
        dw = f1[O_JW + 3 * g:O_JW + 3 * g + 3] - f0[O_JW + 3 * g:O_JW + 3 * g + 3]
        vel += spec.w_joint[g] * dw.dot(dw)
    for e in range(NEE):
        dp = f1[O_EE + 3 * e:O_EE + 3 * e + 3] - f0[O_EE + 3 * e:O_EE + 3 * e + 3]
        row[O_ENDEFF + e] = dp.dot(dp)
    p1 = f1[O_RPOS:O_RPOS + 3].copy(); p1[0] += root_shift[0]; p1[1] += root_shift[1]
    dp = f0[O_RPOS:O_RPOS + 3] - p1
    dv = f1[O_RLIN:O_RLIN + 3] - f0[O_RLIN:O_RLIN + 3]
    dc = f1[O_COMV:O_COMV + 3] - f0[O_COMV:O_COMV + 3]
    row[O_ERR + 0] = row[O_JOINT:O_JOINT + NJ + 1].sum()
    row[O_ERR + 1] = vel
    row[O_ERR + 2] = row[O_ENDEFF:O_ENDEFF + NEE].sum() / NEE
    row[O_ERR + 3] = dp.dot(dp) + 0.1 * th_root ** 2 + 0.01 * dv.dot(dv) + 0.001 * dw_root.dot(dw_root)
    row[O_ERR + 4] = 0.1 * dc.dot(dc)
    row[O_TERM:O_TERM + 5] = TERM_W * np.exp(-TERM_SCALE * row[O_ERR:O_ERR + 5])
    row[O_SUM] = row[O_TERM:O_TERM + 5].sum()
    return row


def terms(spec, table, params, qpos, qvel, frame, cycle=0):
    """the row of one state against table row `frame`, the reference's root shifted by `cycle` completed cycles"""
    shift = (cycle * params[13], cycle * params[14])
    return row_from_features(spec, spec.features(qpos, qvel), table[int(frame)], shift)


def batch_terms(spec, table, params, qpos, qvel, frame, cycle=None):
    cycle = np.zeros(len(qpos), dtype=np.int64) if cycle is None else cycle
    return np.stack([terms(spec, table, params, qpos[i], qvel[i], frame[i], int(cycle[i])) for i in range(len(qpos))])
