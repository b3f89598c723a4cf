"""Float64 restatement of DeepMimic's state features (include/dmenv.h DM_NSTATE; deepmimic_mujoco_amd/state_features.py has the
layout), written from the contract and independent of the package's code: it takes only the compiled model's tables.

Rotations are composed as QUATERNIONS down the tree (root quaternion, then each hinge's axis-angle quaternion in model order) — a
rotation matrix is never converted back to a quaternion, which is ill-conditioned where w is small.  Velocities are the sum over a
body's ancestor dofs: every hinge turns everything below it about its anchor (the frame origin of the body it belongs to), the free
joint translates with qvel[0:3] (world) and turns with qvel[3:6] given in the root's own frame."""
import numpy as np

NSTATE, NBODY = 171, 13
O_PHASE, O_HEIGHT, O_POS, O_VEL = 0, 1, 2, 93


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def qrot(q, v):
    """v rotated by the unit quaternion q:  v + 2 w (u x v) + 2 u x (u x v)"""
    u = q[1:]
    t = 2.0 * np.cross(u, v)
    return v + q[0] * t + np.cross(u, t)


def kinematics(cm, qpos):
    """-> xpos [nb,3] (frame origins), xquat [nb,4] (unit), xipos [nb,3] (centres of mass), axes [nv,3] (world), anchors [nv,3]"""
    nb = cm.nbody
    xpos = np.zeros((nb, 3)); xquat = np.tile([1.0, 0, 0, 0], (nb, 1)); axes = np.zeros((cm.nv, 3)); anchors = np.zeros((cm.nv, 3))
    for b in range(1, nb):
        p = cm.body_parentid[b]
        js = np.nonzero(cm.jnt_bodyid == b)[0]
        if cm.jnt_type[js[0]] == 0:                                   # the free joint
            xpos[b] = qpos[0:3]
            xquat[b] = qpos[3:7] / np.linalg.norm(qpos[3:7])
            for k in range(3):
                axes[k] = np.eye(3)[k]
                axes[3 + k] = qrot(xquat[b], np.eye(3)[k]); anchors[3 + k] = xpos[b]
            continue
        xpos[b] = xpos[p] + qrot(xquat[p], cm.body_pos[b])
        q = xquat[p].copy()
        for j in js:
            d, a = cm.jnt_dofadr[j], cm.jnt_qposadr[j]
            axes[d] = qrot(q, cm.jnt_axis[j]); anchors[d] = xpos[b]
            h = 0.5 * (qpos[a] - cm.qpos0[a])
            q = qmul(q, np.concatenate([[np.cos(h)], np.sin(h) * cm.jnt_axis[j]]))
        xquat[b] = q / np.linalg.norm(q)
    xipos = np.array([xpos[b] + qrot(xquat[b], cm.body_ipos[b]) for b in range(nb)])
    return xpos, xquat, xipos, axes, anchors


_ANC = {}


def ancestor_dofs(cm, b):
    if (id(cm), b) not in _ANC:
        _ANC[(id(cm), b)] = _ancestor_dofs(cm, b)
    return _ANC[(id(cm), b)]


def _ancestor_dofs(cm, b):
    out = []
    while b > 0:
        out += [d for d in range(cm.nv) if cm.dof_bodyid[d] == b]
        b = cm.body_parentid[b]
    return out


def body_velocities(cm, qpos, qvel, kin=None):
    """-> v [nb,3] world velocity of each body's centre of mass, w [nb,3] world angular velocity (kin: kinematics(cm, qpos), if at hand)"""
    xpos, xquat, xipos, axes, anchors = kin if kin is not None else kinematics(cm, qpos)
    v = np.zeros((cm.nbody, 3)); w = np.zeros((cm.nbody, 3))
    for b in range(1, cm.nbody):
        for d in ancestor_dofs(cm, b):
            if d < 3:
                v[b] += axes[d] * qvel[d]
            else:
                w[b] += axes[d] * qvel[d]
                v[b] += np.cross(axes[d], xipos[b] - anchors[d]) * qvel[d]
    return v, w


def heading(root_quat):
    f = qrot(root_quat / np.linalg.norm(root_quat), np.array([1.0, 0, 0]))
    return np.arctan2(f[1], f[0])


def features(cm, qpos, qvel, phase):
    qpos = np.asarray(qpos, dtype=np.float64); qvel = np.asarray(qvel, dtype=np.float64)
    kin = kinematics(cm, qpos)
    xpos, xquat, xipos, _axes, _anchors = kin
    v, w = body_velocities(cm, qpos, qvel, kin)
    hd = heading(qpos[3:7])
    c, s = np.cos(hd), np.sin(hd)
    Rinv = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
    qinv = np.array([np.cos(0.5 * hd), 0, 0, -np.sin(0.5 * hd)])
    f = np.zeros(NSTATE)
    f[O_PHASE] = phase
    f[O_HEIGHT] = xpos[1][2]
    for b in range(1, cm.nbody):
        k = b - 1
        f[O_POS + 7 * k:O_POS + 7 * k + 3] = Rinv @ (xipos[b] - xpos[1])
        q = qmul(qinv, xquat[b])
        f[O_POS + 7 * k + 3:O_POS + 7 * k + 7] = -q if q[0] < 0 else q
        f[O_VEL + 6 * k:O_VEL + 6 * k + 3] = Rinv @ v[b]
        f[O_VEL + 6 * k + 3:O_VEL + 6 * k + 6] = Rinv @ w[b]
    return f


def phase_of(reward_mode, frame_idx, frame_init, n_frames):
    """reward modes 0, 1, 3: frame_idx / n_frames;  2 and 4: ((frame_idx + frame_init) mod n_frames) / n_frames"""
    if reward_mode in (2, 4):
        return ((int(frame_idx) + int(frame_init)) % int(n_frames)) / float(n_frames)
    return int(frame_idx) / float(n_frames)


def batch_features(cm, qpos, qvel, phase):
    return np.stack([features(cm, qpos[i], qvel[i], phase[i]) for i in range(len(qpos))])


QUAT_IDX = np.array([[O_POS + 7 * k + 3 + j for j in range(4)] for k in range(NBODY)])     # [13, 4] columns of the quaternions
W_SMALL = 1e-6


def compare(got, ref, tol_pose, tol_vel):
    """Worst absolute errors (pose block incl. phase and height, velocity block per row against tol_vel [n]) of got against ref,
    both [n, 171].  A quaternion whose reference w is below W_SMALL in magnitude is compared up to sign (the sign rule is
    discontinuous at w = 0).  -> (failures, worst pose error, worst velocity error / bar, number of (state, body) pairs compared up to sign)"""
    got = np.asarray(got, dtype=np.float64).copy(); ref = np.asarray(ref, dtype=np.float64)
    n = len(ref)
    tol_vel = np.broadcast_to(np.asarray(tol_vel, dtype=np.float64), (n,))
    loose = 0
    for i in range(n):
        for k in range(NBODY):
            cols = QUAT_IDX[k]
            if abs(ref[i, cols[0]]) < W_SMALL:
                loose += 1
                if np.abs(got[i, cols] + ref[i, cols]).max() < np.abs(got[i, cols] - ref[i, cols]).max():
                    got[i, cols] = -got[i, cols]
    e_pose = np.abs(got[:, :O_VEL] - ref[:, :O_VEL])
    e_vel = np.abs(got[:, O_VEL:] - ref[:, O_VEL:]) / tol_vel[:, None]
    fails = ["row %d col %d: %.3e" % (i, j, e_pose[i, j]) for i, j in zip(*np.nonzero(~(e_pose <= tol_pose)))]
    fails += ["row %d col %d: %.3e x bar" % (i, O_VEL + j, e_vel[i, j]) for i, j in zip(*np.nonzero(~(e_vel <= 1.0)))]
    return fails, float(e_pose.max()), float(e_vel.max()), loose
