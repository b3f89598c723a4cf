"""Early termination without a GPU: the float64 restatement of the floor-contact rule (tests/floor_numpy.py) against the CPU oracle's
contact list, csrc/floor_contact.h built for the host against that restatement in double and in float, the body sets and their parser, and
the ABI constants."""
import os
import re
import subprocess

import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import termination as T
from tests import floor_numpy as FN
from tests import helpers as H
from tests.emu import hostprog as HP

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEAR_CAP = 0.005               # share of (state, geom) pairs that may lie within FN.BAND of the boundary (the inputs alone: 0.09 %)


def test_query_states_are_the_863_of_the_design():
    q, v = FN.query_states()
    assert q.shape == (863, 35) and v.shape == (863, 34)


def test_restatement_matches_the_cpu_checkers_floor_contacts():
    from oracle import oracle as O
    cm = H.compiled_model()
    q, v = FN.query_states()
    want = FN.masks_of(FN.query_gaps(cm))
    od = O.Data(H.oracle_model())
    bad = []
    for i in range(len(q)):
        od.reset(); od.set_state(q[i], v[i])
        ncon = int(od.get("ncon")[0])
        cg = od.get("contact_geom").reshape(-1, 2).astype(np.int64)[:ncon]
        m = 0
        for g1, g2 in cg:
            if g1 == 0:
                m |= 1 << int(g2)
        if m != int(want[i]):
            bad.append((i, m, int(want[i])))
    assert not bad, bad[:10]
    assert 0 < np.count_nonzero(want) and len(set(want.tolist())) > 20      # (the states exercise the rule: many different contact sets)


def test_inputs_keep_clear_of_the_boundary():
    cm = H.compiled_model()
    gap = np.concatenate([FN.query_gaps(cm), FN.batch_gaps(cm, FN.all_clip_frames())])[:, 1:]
    print("smallest distance from the boundary %.3e m; %d of %d pairs within %.0e m" % (np.abs(gap).min(), (np.abs(gap) <= FN.BAND).sum(), gap.size, FN.BAND))
    assert np.abs(gap).min() > 1e-6
    assert (np.abs(gap) <= FN.BAND).sum() <= NEAR_CAP * gap.size


# ---- csrc/floor_contact.h on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor_host(tmp_path_factory):
    out = HP.build_host("floor_host.cpp", tmp_path_factory.mktemp("floor_host") / "floor_host")
    return out


def host_masks(exe, cm, q, tmp_path, f32=False):
    """csrc/floor_contact.h on cm.kinematics' body frames"""
    vals = [np.array([float(len(q))]), cm.geom_bodyid.astype(np.float64), cm.geom_type.astype(np.float64), cm.geom_pos.reshape(-1), cm.geom_mat.reshape(-1),
            cm.geom_size.reshape(-1), cm.geom_margin.reshape(-1)]
    for i in range(len(q)):
        xpos, xmat = cm.kinematics(q[i])[:2]
        vals += [xpos.reshape(-1), xmat.reshape(-1)]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate(vals).astype(np.float64).tofile(fin)
    subprocess.check_call([exe, fin, fout] + (["32"] if f32 else []))
    return np.fromfile(fout, dtype=np.float64).astype(np.int32)


@pytest.fixture(scope="module")
def wide():
    """the 863 query states plus every frame of all 15 clips, with the restatement's gaps"""
    cm = H.compiled_model()
    q = np.concatenate([FN.query_states()[0], FN.all_clip_frames()])
    return cm, q, np.concatenate([FN.query_gaps(cm), FN.batch_gaps(cm, FN.all_clip_frames())])


def test_floor_contact_h_in_double_is_exact(floor_host, wide, tmp_path):
    cm, q, gap = wide
    got = host_masks(floor_host, cm, q, tmp_path)
    np.testing.assert_array_equal(got, FN.masks_of(gap))


def test_floor_contact_h_in_float_differs_only_inside_the_band(floor_host, wide, tmp_path):
    cm, q, gap = wide
    got = host_masks(floor_host, cm, q, tmp_path, f32=True)
    wrong, near = FN.compare(got, gap)
    pairs = gap[:, 1:].size
    print("host float32: %d of %d pairs within %.0e m of the boundary (%.3f %%), %d of them decided differently"
          % (near, pairs, FN.BAND, 100.0 * near / pairs, int((got != FN.masks_of(gap)).sum())))
    assert near <= NEAR_CAP * pairs
    assert not wrong, wrong[:10]


# ---- body sets, parser, reason bits -------------------------------------------------------------------------------------------------
def test_body_sets_and_parser():
    names = H.compiled_model().body_names
    assert tuple(names) == T.BODY_NAMES and len(names) == 14
    dm = T.fall_body_mask("deepmimic")
    assert dm == sum(1 << b for b in range(1, 14) if names[b] not in ("right_ankle", "left_ankle")) and bin(dm).count("1") == 11
    assert T.fall_body_mask("crawl") == (1 << names.index("root")) | (1 << names.index("chest")) | (1 << names.index("neck")) == 0b1110
    assert T.fall_body_mask(None) == T.fall_body_mask("none") == T.fall_body_mask(()) == 0
    assert T.fall_body_mask(["root", 3, "left_knee"]) == (1 << 1) | (1 << 3) | (1 << names.index("left_knee"))
    assert T.fall_body_mask("neck") == 1 << 3 and T.fall_body_mask(0b1010) == 0b1010
    for bad in (["pelvis"], "torso", [0], [14], 1, 1 << 14):
        with pytest.raises(ValueError):
            T.fall_body_mask(bad)
    cm = H.compiled_model()
    g = T.geoms_of_bodies(T.fall_body_mask("deepmimic"), cm.geom_bodyid)
    ankles = [i for i in range(cm.ngeom) if names[cm.geom_bodyid[i]] in ("right_ankle", "left_ankle")]
    assert g == sum(1 << i for i in range(1, cm.ngeom) if i not in ankles) and len(ankles) == 2


def test_reason_bits():
    assert (T.DONE_STEP, T.DONE_FALL, T.DONE_TIME_LIMIT) == (A.DONE_STEP, A.DONE_FALL, A.DONE_TIME_LIMIT) == (1, 2, 4)
    assert T.reason_names(0) == [] and T.reason_names(6) == ["fall", "time_limit"] and T.reason_names(1) == ["step"]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_header_and_python_mirror_agree_on_the_new_ids():
    hdr = open(os.path.join(ROOT, "include", "dmenv.h")).read()
    for name, val in [("DM_OPT_FALL_BODIES", A.OPT_FALL_BODIES), ("DM_OPT_MAX_EPISODE_STEPS", A.OPT_MAX_EPISODE_STEPS), ("DM_F_EPISODE_STEPS", A.F_EPISODE_STEPS),
                      ("DM_F_DONE_REASON", A.F_DONE_REASON)]:
        assert int(re.search(r"%s = (\d+)" % name, hdr).group(1)) == val
    for name, val in [("DM_DONE_STEP", A.DONE_STEP), ("DM_DONE_FALL", A.DONE_FALL), ("DM_DONE_TIME_LIMIT", A.DONE_TIME_LIMIT)]:
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val
    assert (A.OPT_FALL_BODIES, A.OPT_MAX_EPISODE_STEPS, A.F_EPISODE_STEPS, A.F_DONE_REASON) == (9, 10, 17, 18)
    assert A.FIELD_SPEC[A.F_EPISODE_STEPS] == (np.int32, ()) and A.FIELD_SPEC[A.F_DONE_REASON] == (np.int32, ())
    assert "int dm_batch_floor_contacts(" in hdr


@pytest.mark.parametrize("dtype", [64, 32])
def test_both_libraries_export_the_query(dtype):
    L = A.load(dtype)
    assert "dm_batch_floor_contacts" in A.EXPORTS and hasattr(L, "dm_batch_floor_contacts")
    assert L.dm_batch_floor_contacts(None, None, None, 4, None, A.PTR_HOST) == -1 and b"null" in L.dm_last_error()      # (refused before any device is touched)
