"""TEST INFRASTRUCTURE: the restatement of an external push in numpy (include/dmenv.h "EXTERNAL PUSHES"):  dqvel = M(q)^-1 J_b(q)^T p.
J_b is built from the CPU oracle's kinematics (xpos, xmat, xipos through dmo_data_get) and the compiled model's joint axes, and the system is solved with
the oracle's M (armature included).  test_push.py checks J_b itself against central differences of the oracle's xipos."""
import numpy as np

from deepmimic_mujoco_amd.model import _axis_angle_mat


def oracle_kinematics(od, q, v=None):
    """set the state (which runs the oracle's forward evaluation) -> xpos [14,3], xmat [14,3,3], xipos [14,3], M [34,34] as float64"""
    od.set_state(q, np.zeros(34) if v is None else v)
    return od.get("xpos").reshape(14, 3), od.get("xmat").reshape(14, 3, 3), od.get("xipos").reshape(14, 3), od.get("M").reshape(34, 34)


def jacobian(cm, q, xpos, xmat, xipos, b, dtype=np.float64):
    """J_b [3,34]: the translational Jacobian of the point xipos[b] in the dofs of qvel.  Hinge dof d of a body c on the chain root -> b: axis_world_d x
    (xipos_b - xpos_c), where a body's hinges turn one after the other (hinge k's world axis is the parent's frame times the body's earlier hinge rotations
    times the model's axis); root translation: identity; root rotation (body-frame angular velocity): xmat_root[:, k] x (xipos_b - xpos_root)."""
    f = dtype
    q = np.asarray(q, dtype=f); xpos = np.asarray(xpos, dtype=f); xmat = np.asarray(xmat, dtype=f); xipos = np.asarray(xipos, dtype=f)
    J = np.zeros((3, cm.nv), dtype=f)
    c = int(b)
    while c > 0:
        r = xipos[b] - xpos[c]
        js = np.nonzero(cm.jnt_bodyid == c)[0]
        if c == 1:
            J[:, 0:3] = np.eye(3, dtype=f)
            for k in range(3):
                J[:, 3 + k] = np.cross(xmat[1][:, k], r)
        else:
            R = xmat[cm.body_parentid[c]].copy()
            for j in js:
                qa, da = cm.jnt_qposadr[j], cm.jnt_dofadr[j]
                ax = cm.jnt_axis[j].astype(f)
                J[:, da] = np.cross(R @ ax, r)
                R = (R @ _axis_angle_mat(cm.jnt_axis[j], float(q[qa]) - cm.qpos0[qa]).astype(f)).astype(f)
        c = int(cm.body_parentid[c])
    return J


def push_dqvel(cm, od, q, b, p, dtype=np.float64):
    """dqvel [34] of the impulse p on body b at pose q, evaluated in `dtype` (od: an oracle Data of the matching build for float32)"""
    xpos, xmat, xipos, M = oracle_kinematics(od, q)
    J = jacobian(cm, q, xpos, xmat, xipos, b, dtype)
    rhs = (J.T @ np.asarray(p, dtype=dtype)).astype(dtype)
    return np.linalg.solve(M.astype(dtype), rhs).astype(dtype)


def quat_mul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def moved(q, d, eps):
    """q after the dof d of qvel has moved by eps: translation and hinges through qpos, root rotation through q (x) exp(eps e_k / 2)"""
    q = np.array(q, dtype=np.float64)
    q[3:7] /= np.linalg.norm(q[3:7])
    if d < 3:
        q[d] += eps
    elif d < 6:
        h = np.zeros(4); h[0] = np.cos(eps / 2); h[1 + d - 3] = np.sin(eps / 2)
        q[3:7] = quat_mul(q[3:7], h)
    else:
        q[d + 1] += eps
    return q


def jacobian_fd(od, q, b, eps=1e-6):
    """central differences of the oracle's xipos[b] over the 34 dofs"""
    J = np.zeros((3, 34))
    for d in range(34):
        hi = oracle_kinematics(od, moved(q, d, eps))[2][b].copy()
        lo = oracle_kinematics(od, moved(q, d, -eps))[2][b].copy()
        J[:, d] = (hi - lo) / (2 * eps)
    return J
