"""Float64 restatement of the floor-contact rule (include/dmenv.h dm_batch_floor_contacts; csrc/floor_contact.h) on `CompiledModel.kinematics`:
geom g touches the floor when the collision stage would emit a contact for (floor geom 0, g).  `gaps` gives each geom's signed distance from
that decision's boundary (<= 0: touches), which the float32 tests use to tell pairs that may legitimately differ."""
import numpy as np

from deepmimic_mujoco_amd.model import GEOM_TYPES

SPHERE, CAPSULE, BOX = GEOM_TYPES["sphere"], GEOM_TYPES["capsule"], GEOM_TYPES["box"]
BAND = 1e-4                   # pairs this close to the boundary (metres) may differ in float32
CORNERS = np.array([[(-1, 1)[i & 1], (-1, 1)[(i >> 1) & 1], (-1, 1)[(i >> 2) & 1]] for i in range(8)], dtype=np.float64)


def gaps(cm, q):
    """[ngeom] signed distance of every geom's test from its boundary at qpos q (entry 0, the floor itself, is +inf)"""
    xpos, xmat = cm.kinematics(np.asarray(q, dtype=np.float64))[:2]
    gb = cm.geom_bodyid
    gpos = xpos[gb] + np.einsum("gij,gj->gi", xmat[gb], cm.geom_pos)
    gmat = np.einsum("gij,gjk->gik", xmat[gb], cm.geom_mat)
    p0, n = gpos[0], gmat[0][:, 2]
    out = np.full(cm.ngeom, np.inf)
    for g in range(1, cm.ngeom):
        margin = max(cm.geom_margin[0], cm.geom_margin[g])
        t, size = cm.geom_type[g], cm.geom_size[g]
        if t == SPHERE:
            out[g] = n @ (gpos[g] - p0) - (margin + size[0])
        elif t == CAPSULE:
            ax = gmat[g][:, 2]
            out[g] = min(n @ (gpos[g] + s * ax * size[1] - p0) - (margin + size[0]) for s in (1.0, -1.0))
        elif t == BOX:
            dist = n @ (gpos[g] - p0)
            ld = (CORNERS * size) @ gmat[g].T @ n
            out[g] = np.min(np.maximum(dist + ld - margin, ld))       # a corner counts when ld <= 0 and dist + ld <= margin
    return out


def batch_gaps(cm, qs):
    return np.stack([gaps(cm, q) for q in qs])


def masks_of(gap):
    """[n] int32 bit masks from [n, ngeom] gaps"""
    return ((gap <= 0) * (1 << np.arange(gap.shape[1]))).sum(1).astype(np.int32)


def floor_masks(cm, qs):
    return masks_of(batch_gaps(cm, qs))


def compare(got, gap, band=BAND):
    """(wrong, near): (state, geom) pairs where mask `got` disagrees with the restatement outside the band, and the number of pairs inside it"""
    bits = (np.asarray(got)[:, None] >> np.arange(gap.shape[1])) & 1
    want = gap <= 0
    near = np.abs(gap) <= band
    wrong = np.argwhere((bits.astype(bool) != want) & ~near)
    return [tuple(w) for w in wrong], int(near[:, 1:].sum())


CLIPS = ("walk", "cartwheel", "getup_faceup", "crawl")
ALL_CLIPS = ("backflip", "cartwheel", "crawl", "dance_a", "dance_b", "getup_facedown", "getup_faceup", "jump", "kick", "punch", "roll", "run", "spin",
             "spinkick", "walk")
_STATES = {}


def query_states():
    """(qpos, qvel) of the bar tests: varied_states(256, seed=3), then every frame of walk, cartwheel, getup_faceup and crawl — 863 states"""
    from tests import helpers as H
    if "bar" not in _STATES:
        _idx, q, v, _ws, _ctrl = H.varied_states(256, seed=3)
        qs, vs = [q], [v]
        for clip in CLIPS:
            mc = H.mocap(clip)
            qs.append(mc.data_config); vs.append(mc.data_vel)
        _STATES["bar"] = (np.concatenate(qs), np.concatenate(vs))
    return _STATES["bar"]


def all_clip_frames():
    from tests import helpers as H
    if "clips" not in _STATES:
        _STATES["clips"] = np.concatenate([H.mocap(c).data_config for c in ALL_CLIPS])
    return _STATES["clips"]


def query_gaps(cm):
    """the restatement on query_states(), computed once"""
    if "gaps" not in _STATES:
        _STATES["gaps"] = batch_gaps(cm, query_states()[0])
    return _STATES["gaps"]
