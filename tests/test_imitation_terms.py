"""The imitation reward's terms row without a GPU: the float64 restatement (tests/terms_numpy.py) against the oracle and its own sum
identities, the kernel's lane code (csrc/env_step.h imitation_reward<R, true>) built for the host on the wave testbench
(tests/terms_host.cpp) against that restatement in double and in float, the ABI, `Batch.imitation_terms`' argument rules and the staging
layout of the fourth view under the sanitizers (tests/terms_stage_host.cpp).

Bars.  Double: 1e-9 absolute on every column (no column of the states below exceeds a few hundred; the rows that matter are O(1)).
Float: per column, FLOAT_MARGIN = 4 times the largest |float32 oracle - float64 oracle| over the same states — the wave's butterfly sums add
in another order than the oracle's serial loops.  The oracle returns the five errors and the reward (columns 0..4 and 10); the columns it
does not return take their bar from the column they add up to, which they cannot move by more than they move themselves:
  [5..10)   w_k exp(-s_k e_k): |d term| <= w_k s_k |d e_k|, plus one float rounding of a value <= w_k      -> w_k s_k bar[k] + w_k 2^-23
  [11..24)  the shares of the pose error, each >= 0 and formed like the sum they add up to                  -> bar[0]
  [24..28)  the end effectors' squared distances, whose sum / 4 is column 2                                -> 4 bar[2]
The observed ratios are recorded in profiles/terms_kernels.md."""
import os
import subprocess

import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import imitation as IM
from deepmimic_mujoco_amd.batch import Batch
from tests import helpers as H
from tests.emu import hostprog as HP
from tests import terms_numpy as TN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL64 = 1e-9
FLOAT_MARGIN = 4.0
_CASES = {}


def spec():
    return IM.ImitationSpec(H.compiled_model())


def cases(clip="walk"):
    """The states every comparison of the view uses -> dict(table, params, qpos, qvel, frame, cycle, names): every frame of the clip against
    its own row and against the next row, 32 seeded perturbations, a negated root quaternion, a 1e-7 rad turn of one ball joint (the zero
    branch of quat_diff_theta), and cycle = 2 on the wrapping clip."""
    if clip in _CASES:
        return _CASES[clip]
    sp = spec(); mc = H.mocap(clip)
    table, params = sp.table_for(mc)
    rv = sp.reference_qvel(mc.data_config, np.asarray(mc.data)[:, 0], mc.loop)
    F = len(table)
    qs, vs, fr, cy, names = [], [], [], [], []

    def add(q, v, k, c, name):
        qs.append(np.array(q, dtype=np.float64)); vs.append(np.array(v, dtype=np.float64)); fr.append(int(k)); cy.append(int(c)); names.append(name)
    for k in range(F):
        add(mc.data_config[k], rv[k], k, 0, "own row")
    for k in range(F):
        add(mc.data_config[k], rv[k], (k + 1) % F, 0, "next row")
    idx, q, v, _ws, _ctrl = H.varied_states(32, seed=21, clip=clip)
    for e in range(32):
        add(q[e], v[e], idx[e], 0, "perturbed")
    k = 9
    qb = mc.data_config[k].copy(); qb[7:] += 0.05
    qn = qb.copy(); qn[3:7] = -qn[3:7]
    add(qb, rv[k], k + 1, 0, "root quaternion")
    add(qn, rv[k], k + 1, 0, "negated root quaternion")
    qt = mc.data_config[k].copy(); qt[7 + 14] += 1e-7                    # one hinge of the right hip's triple
    add(qt, rv[k], k, 0, "1e-7 rad on a ball joint")
    assert mc.loop == "wrap" and np.abs(params[13:15]).max() > 0.1
    qc = mc.data_config[3].copy(); qc[0:2] += 2 * params[13:15]; qc[7:] += 0.02
    add(qc, rv[3], 3, 2, "cycle 2")
    add(qc, rv[3], 3, 0, "cycle 0, same state")
    out = dict(table=table, params=params, qpos=np.stack(qs), qvel=np.stack(vs), frame=np.array(fr, dtype=np.int32), cycle=np.array(cy, dtype=np.int32),
               names=names, n_frames=F)
    out["ref"] = TN.batch_terms(sp, table, params, out["qpos"], out["qvel"], out["frame"], out["cycle"])
    _CASES[clip] = out
    return out


_ORACLE = {}


def oracle_rows(dtype):
    """[n, 6]: the oracle's five errors and its reward for cases(), in the oracle build of arithmetic `dtype`"""
    if dtype not in _ORACLE:
        from oracle import oracle as O
        c = cases()
        om = O.Model(dtype=dtype)
        rows = []
        for i in range(len(c["qpos"])):
            f0 = O.imitation_features(om, c["qpos"][i], c["qvel"][i], c["params"])
            shift = (c["cycle"][i] * c["params"][13], c["cycle"][i] * c["params"][14])
            r, t5 = O.imitation_reward(om, f0, c["table"][c["frame"][i]], c["params"], shift=shift)
            rows.append(np.concatenate([t5, [r]]))
        _ORACLE[dtype] = np.stack(rows)
    return _ORACLE[dtype]


ORACLE_COLS = [0, 1, 2, 3, 4, 10]


def float_bars():
    """[28] the float32 bar of each column (this file's docstring), from the two oracle builds"""
    d = np.abs(oracle_rows(32) - oracle_rows(64)).max(0)
    assert (d > 0).all() and (d < 1e-2).all(), d
    bar = np.zeros(TN.NTERMS)
    bar[0:5] = FLOAT_MARGIN * d[0:5]
    bar[10] = FLOAT_MARGIN * d[5]
    bar[5:10] = IM.TERM_W * IM.TERM_SCALE * bar[0:5] + IM.TERM_W * 2.0 ** -23
    bar[11:24] = bar[0]
    bar[24:28] = 4 * bar[2]
    return bar


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_oracle_and_its_own_sums():
    c = cases()
    ref, orc = c["ref"], oracle_rows(64)
    assert ref.shape == (len(c["qpos"]), 28) and np.isfinite(ref).all()
    err = np.abs(ref[:, ORACLE_COLS] - orc)
    print("restatement against the oracle: worst %.3e" % err.max())
    assert err.max() <= TOL64
    np.testing.assert_allclose(ref[:, 11:24].sum(1), ref[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref[:, 24:28].sum(1) / 4, ref[:, 2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref[:, 5:10].sum(1), ref[:, 10], rtol=0, atol=1e-15)
    sp = spec()
    for i in (0, 50, len(ref) - 1):                                      # the package's own numpy path says the same
        f0 = sp.features(c["qpos"][i], c["qvel"][i])
        sh = (c["cycle"][i] * c["params"][13], c["cycle"][i] * c["params"][14])
        np.testing.assert_allclose(ref[i, 0:5], sp.reward_terms(f0, c["table"][c["frame"][i]], sh), rtol=0, atol=1e-12)


def test_known_rows():
    c = cases()
    ref, names = c["ref"], c["names"]
    own = [i for i, nm in enumerate(names) if nm == "own row"]
    assert len(own) == c["n_frames"]
    assert np.abs(ref[own, 0:5]).max() < 1e-20 and np.abs(ref[own, 11:28]).max() < 1e-20          # errors 0 ...
    np.testing.assert_allclose(ref[own, 5:10], np.tile(IM.TERM_W, (len(own), 1)), rtol=0, atol=1e-15)   # ... terms equal to the weights ...
    np.testing.assert_allclose(ref[own, 10], 1.0, rtol=0, atol=1e-15)                                # ... reward 1
    nxt = [i for i, nm in enumerate(names) if nm == "next row"]
    assert (ref[nxt, 0] > 0).all() and (ref[nxt, 10] < 1).all()
    a, b = names.index("root quaternion"), names.index("negated root quaternion")
    np.testing.assert_allclose(ref[a], ref[b], rtol=0, atol=1e-12)
    t = names.index("1e-7 rad on a ball joint")
    hip = list(H.compiled_model().body_names).index("right_hip") - 2
    assert ref[t, 11 + hip] == 0.0 and ref[t, 0] == 0.0 and ref[t, 2] > 0                            # the angle reads as zero, the foot has moved
    cy, c0 = names.index("cycle 2"), names.index("cycle 0, same state")
    assert ref[cy, 3] < 1e-20 and ref[c0, 3] > 1.0 and np.array_equal(ref[cy, 11:28], ref[c0, 11:28])


def test_reward_from_errors():
    c = cases()
    ref = c["ref"]
    np.testing.assert_allclose(IM.reward_from_errors(ref[:, 0:5]), ref[:, 10], rtol=0, atol=1e-15)
    w = np.array([0.3, 0.1, 0.2, 0.3, 0.1]); s = np.array([1.0, 0.2, 20.0, 4.0, 8.0])
    np.testing.assert_allclose(IM.reward_from_errors(ref[:, 0:5], w, s), (w * np.exp(-s * ref[:, 0:5])).sum(1), rtol=0, atol=1e-15)
    import torch
    t = IM.reward_from_errors(torch.as_tensor(ref[:, 0:5]))
    assert t.dtype == torch.float64 and tuple(t.shape) == (len(ref),)
    np.testing.assert_allclose(t.numpy(), ref[:, 10], rtol=0, atol=1e-15)
    assert IM.TERM_NAMES == ("pose", "velocity", "end_effector", "root", "com") and IM.NTERMS == 28 == A.NTERMS == TN.NTERMS
    assert (IM.O_TERM_ERR, IM.O_TERM_VALUE, IM.O_TERM_REWARD, IM.O_TERM_JOINT, IM.O_TERM_ENDEFF) == (0, 5, 10, 11, 24)


# ---- the lane code on the wave testbench ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terms_host(tmp_path_factory):
    out = HP.build_host("terms_host.cpp", tmp_path_factory.mktemp("terms_host") / "terms_host", testbench=True, opt=("-O1", "-g"))
    return out


def host_terms(exe, c, tmp_path, f32=False, frame=None):
    cm = H.compiled_model()
    n = len(c["qpos"])
    frame = c["frame"] if frame is None else frame
    per = np.concatenate([c["qpos"], c["qvel"], np.asarray(frame, dtype=np.float64)[:, None], c["cycle"].astype(np.float64)[:, None]], 1)
    vals = np.concatenate([[float(n), float(c["n_frames"])], np.asarray(cm.body_pos, dtype=np.float64).reshape(-1), np.asarray(cm.body_ipos, dtype=np.float64).reshape(-1),
                           np.asarray(cm.body_mass, dtype=np.float64).reshape(-1), np.asarray(cm.body_inertia, dtype=np.float64).reshape(-1),
                           np.asarray(cm.jnt_axis, dtype=np.float64).reshape(-1), c["params"], c["table"].reshape(-1), per.reshape(-1)])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    vals.tofile(fin)
    subprocess.check_call([exe, fin, fout] + (["32"] if f32 else []))
    return np.fromfile(fout, dtype=np.float64).reshape(n, TN.NTERMS)


def test_lane_code_in_double_matches_the_restatement(terms_host, tmp_path):
    c = cases()
    got = host_terms(terms_host, c, tmp_path)
    err = np.abs(got - c["ref"])
    print("host double: worst error %.3e (column %d)" % (err.max(), int(err.max(0).argmax())))
    assert err.max() <= TOL64
    assert np.abs(got[:, ORACLE_COLS] - oracle_rows(64)).max() <= TOL64
    own = [i for i, nm in enumerate(c["names"]) if nm == "own row"]
    assert np.abs(got[own, 10] - 1.0).max() <= 1e-12
    a, b = c["names"].index("root quaternion"), c["names"].index("negated root quaternion")
    assert np.abs(got[a] - got[b]).max() <= 1e-12
    bad = c["frame"].copy(); bad[1] = c["n_frames"]; bad[4] = -1           # a frame outside the table: a NaN row, its neighbours untouched
    nan = host_terms(terms_host, c, tmp_path, frame=bad)
    assert np.isnan(nan[[1, 4]]).all() and np.array_equal(np.delete(nan, [1, 4], 0), np.delete(got, [1, 4], 0))


def test_lane_code_in_float_stays_inside_the_oracle_derived_bars(terms_host, tmp_path):
    c = cases()
    bar = float_bars()
    got = host_terms(terms_host, c, tmp_path, f32=True)
    ratio = (np.abs(got - c["ref"]) / bar).max(0) * FLOAT_MARGIN       # in units of the oracles' own difference
    print("host float: worst error per column, as a multiple of the largest |oracle32 - oracle64| (bar: %g):\n%s" % (FLOAT_MARGIN, np.array2string(ratio, precision=3)))
    print("bars: %s" % np.array2string(bar, precision=3))
    assert (ratio <= FLOAT_MARGIN).all(), ratio


# ---- the ABI and the Python method ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [64, 32])
def test_both_libraries_export_the_entry_point(dtype):
    L = A.load(dtype)
    assert L.dm_abi_version() == 9 == A.ABI_VERSION and A.NTERMS == 28
    assert "dm_batch_imitation_terms" in A.EXPORTS and hasattr(L, "dm_batch_imitation_terms")
    hdr = open(os.path.join(ROOT, "include", "dmenv.h")).read()
    assert "#define DM_ABI_VERSION 9" in hdr and "#define DM_NTERMS 28" in hdr and "int dm_batch_imitation_terms(" in hdr


class _StubLib(object):
    def __init__(self):
        self.calls = []

    def dm_batch_imitation_terms(self, *a):
        self.calls.append(a)
        return 0


def stub_batch(n=6):
    b = Batch.__new__(Batch)                                              # no library, no device: a stub takes the call
    b.n, b.device, b._L, b._h = n, 0, _StubLib(), None
    return b


def test_method_takes_n_from_the_state_then_env_ids_then_the_batch():
    b = stub_batch()
    q, v, f = np.zeros((18, A.NQ)), np.zeros((18, A.NV)), np.zeros(18, dtype=np.int32)
    out = b.imitation_terms(qpos=q, qvel=v, frame=f)
    _h, qp, vp, fp, cp, ip, n, op, kind = b._L.calls[-1]
    assert n == 18 and out.shape == (18, 28) and out.dtype == np.float64 and kind == A.PTR_HOST
    assert qp.value == q.ctypes.data and fp.value == f.ctypes.data and cp is None and ip is None and op.value == out.ctypes.data
    b.imitation_terms(qpos=q, qvel=v, frame=f, cycle=np.ones(18, dtype=np.int64))
    assert b._L.calls[-1][4] is not None
    assert b.imitation_terms(env_ids=np.array([4, 1], dtype=np.int32)).shape == (2, 28)
    _h, qp, vp, fp, cp, ip, n, op, kind = b._L.calls[-1]
    assert n == 2 and qp is None and vp is None and fp is None and cp is None and ip is not None
    assert b.imitation_terms().shape == (6, 28) and b._L.calls[-1][6] == 6 and b._L.calls[-1][5] is None
    given = np.full((6, 28), 7.0)
    assert b.imitation_terms(out=given) is given and b._L.calls[-1][7].value == given.ctypes.data


def test_method_refuses_bad_arguments_before_the_library():
    b = stub_batch()
    q, v, f = np.zeros((2, A.NQ)), np.zeros((2, A.NV)), np.zeros(2, dtype=np.int32)
    for kw in (dict(qpos=q), dict(qpos=q, qvel=v), dict(qvel=v, frame=f), dict(frame=f), dict(cycle=f), dict(qpos=q, frame=f)):      # a partial explicit state
        with pytest.raises(ValueError):
            b.imitation_terms(**kw)
    with pytest.raises(ValueError):
        b.imitation_terms(qpos=q, qvel=v, frame=f, env_ids=[0, 1])      # an explicit state excludes env_ids
    with pytest.raises(ValueError):
        b.imitation_terms(qpos=q, qvel=v, frame=np.zeros(3, dtype=np.int32))
    for bad in (np.zeros((5, 28)), np.zeros((6, 29)), np.zeros(6 * 28), np.zeros((6, 28), dtype=np.float32), np.zeros((28, 6)).T):
        with pytest.raises(ValueError):
            b.imitation_terms(out=bad)
    assert b._L.calls == []


# ---- the fourth view's staging layout, under the sanitizers ------------------------------------------------------------------------------
def test_terms_staging_layout_under_the_sanitizers(tmp_path):
    exe = HP.build_host("terms_stage_host.cpp", tmp_path / "terms_stage_host", sanitize=True, opt=("-O1", "-g"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 5 sizes x 2 callers x 2^6 presence masks of the six arrays dm_batch_imitation_terms declares
    assert r.stdout.strip() == "terms_stage_host: %d layouts hold" % (5 * 2 * 64), r.stdout
