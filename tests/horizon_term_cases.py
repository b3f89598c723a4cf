"""Inputs shared by tests/test_horizon_termination.py (the wave-testbench twin) and tests/test_gpu_horizon_termination.py: the states, actions and the
input condition of the comparisons between early termination behind step launches and inside the horizon launch (DM_OPT_HORIZON_TERMINATION)."""
import numpy as np

from tests import floor_numpy as FN
from tests import helpers as H

STATE_SEED, ACTION_SEED = 5, 3
STATE_SEED32 = 5           # the float32 case's states: its band is five orders of magnitude wider, and the seed is the one whose decisions stay outside it
MANY_ROW_ENVS = (3, 6)        # where the two many-row states go (not among the sunk frames 0, 8, 16, ...)
# The slot kinematics (four environments per wavefront) and the one-env kinematics differ in the last bits (other summation orders), so a fall decision
# whose geom lies closer to the rule's boundary than this is not defined between the two forms: the inputs must hold no such pair.  1e-9 m is the
# agreement bar of the two kernels' positions with the oracle.
BOUNDARY = 1e-9
BOUNDARY32 = FN.BAND          # the float32 library's band (tests/test_gpu_termination.py)
_MANY = {}


def many_rows():
    if "s" not in _MANY:
        _MANY["s"] = H.many_row_states(40, 64, want=2)
    return _MANY["s"]


def states(n, many=True, seed=STATE_SEED):
    """helpers.varied_states(n, seed=5), every other exact mocap frame (env 0, 8, ...) sunk 0.10 m so that a shin touches the floor while the centre of
    mass stays inside the step's band, and — `many` — two states with more than 40 constraint rows, which the packed step hands to the one-env code"""
    idx, q, v, _ws, _c = H.varied_states(n, seed=seed)
    q[0::8, 2] -= 0.10
    if many:
        mi, mq, mv = many_rows()
        for k, e in enumerate(MANY_ROW_ENVS):
            idx[e], q[e], v[e] = mi[k], mq[k], mv[k]
    return idx, q, v


def actions(T, n):
    return np.random.RandomState(ACTION_SEED).randn(T, n, 28) * 0.9


def closest_decision(cm, qpos, tested, geoms=None):
    """the smallest |gap| over the (state, geom) pairs of the tested states: qpos [..., 35], tested [...] bool; `geoms`: a bit mask of the geoms that
    decide (those of the fall set's bodies; None: all fifteen)"""
    q = np.asarray(qpos).reshape(-1, 35)[np.asarray(tested).reshape(-1)]
    if len(q) == 0:
        return np.inf
    gap = np.abs(FN.batch_gaps(cm, q))
    which = [g for g in range(1, gap.shape[1]) if geoms is None or (int(geoms) >> g) & 1]
    return float(gap[:, which].min())
