"""The host side the three read-only views share, without a GPU: batch._view_args on numpy arrays (no library is loaded: Batch._ptr needs
its object only for tensors), and csrc/view_stage.h built for the host under the address and undefined-behaviour sanitizers
(tests/stage_host.cpp)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd.batch import Batch, _view_args
from tests.emu import hostprog as HP

N_BATCH = 6
F64, I32 = np.float64, np.int32


def call(state, env_ids, outs, who="view"):
    return _view_args(lambda *a, **kw: Batch._ptr(None, *a, **kw), N_BATCH, 0, state, env_ids, outs, who)


def state_of(n=None):
    if n is None:
        return [(None, F64, (A.NQ,)), (None, F64, (A.NV,)), (None, F64, ())]
    return [(np.zeros((n, A.NQ)), F64, (A.NQ,)), (np.zeros((n, A.NV)), F64, (A.NV,)), (np.zeros(n), F64, ())]


def test_n_comes_from_the_state_then_env_ids_then_the_batch():
    outs = [(None, F64, (A.NSTATE,))]
    assert call(state_of(18), None, outs)[0] == 18                    # explicit states may outnumber the batch
    assert call(state_of(), np.array([4, 1], dtype=I32), outs)[0] == 2
    assert call(state_of(), [5, 0, 5], outs)[0] == 3                  # (a list will do)
    assert call(state_of(), None, outs)[0] == N_BATCH
    assert call([], None, outs)[0] == N_BATCH                         # a view without an explicit-state form


def test_outputs_are_allocated_with_dtype_and_shape():
    specs = [(None, np.uint8, (8, 9, 3)), (None, np.float32, (8, 9)), (None, I32, (8, 9)), (None, F64, (A.NGEOM, 12)), (None, I32, ())]
    n, ins, ptrs, kind, keep, objs = call([(None, F64, (A.NQ,))], np.array([4, 1], dtype=I32), specs)
    assert n == 2 and kind == A.PTR_HOST and len(ptrs) == len(objs) == 5
    for (_x, dt, shp), p, o in zip(specs, ptrs, objs):
        assert isinstance(o, np.ndarray) and o.dtype == dt and o.shape == (2,) + shp and o.flags.c_contiguous
        assert p.value == o.ctypes.data
    assert any(k is objs[0] for k in keep)                            # what a pointer points into is kept alive
    given = np.full((N_BATCH, A.NSTATE), 7.0)
    n, _ins, (p,), kind, _keep, (o,) = call(state_of(), None, [(given, F64, (A.NSTATE,))])
    assert o is given and p.value == given.ctypes.data and (given == 7.0).all()


def test_inputs_become_pointers_and_none_stays_null():
    q = np.arange(3 * A.NQ, dtype=F64).reshape(3, A.NQ)
    n, (qp, ip), _outs, kind, keep, _objs = call([(q, F64, (A.NQ,))], None, [(None, I32, ())])
    assert n == 3 and qp.value == q.ctypes.data and ip is None and kind == A.PTR_HOST
    n, (qp, vp, pp, ip), _outs, kind, keep, _objs = call(state_of(), None, [(None, F64, (A.NSTATE,))])
    assert qp is None and vp is None and pp is None and ip is None
    ids = [4, 1]                                                      # converted: the pointer is into the keepalive, int32
    n, (qp, ip), _outs, kind, keep, _objs = call([(None, F64, (A.NQ,))], ids, [(None, I32, ())])
    held = [k for k in keep if k is not None and k.dtype == I32 and k.shape == (2,) and ip.value == k.ctypes.data]
    assert qp is None and len(held) == 1 and held[0].tolist() == ids
    q32 = np.ones((2, A.NQ), dtype=np.float32)                        # inputs are converted to the dtype the library reads
    n, (qp, ip), _outs, _kind, keep, _objs = call([(q32, F64, (A.NQ,))], None, [(None, I32, ())])
    assert (C.c_double * (2 * A.NQ)).from_address(qp.value)[:] == [1.0] * (2 * A.NQ)


def test_an_explicit_state_excludes_env_ids():
    with pytest.raises(ValueError):
        call(state_of(2), np.zeros(2, dtype=I32), [(None, F64, (A.NSTATE,))])
    with pytest.raises(ValueError):
        call([(np.zeros((1, A.NQ)), F64, (A.NQ,))], [0], [(None, I32, ())])


@pytest.mark.parametrize("bad", [np.zeros((5, A.NSTATE)), np.zeros((N_BATCH, A.NSTATE + 1)), np.zeros(N_BATCH * A.NSTATE), np.zeros((N_BATCH, A.NSTATE), dtype=np.float32),
                                 np.zeros((N_BATCH, A.NSTATE), dtype=I32), np.zeros((A.NSTATE, N_BATCH)).T])
def test_a_given_output_of_the_wrong_shape_dtype_or_layout_is_refused(bad):
    with pytest.raises(ValueError):
        call(state_of(), None, [(bad, F64, (A.NSTATE,))])


def test_an_input_of_the_wrong_shape_is_refused():
    with pytest.raises(ValueError):
        call([(np.zeros((3, A.NQ + 1)), F64, (A.NQ,))], None, [(None, I32, ())])
    with pytest.raises(ValueError):
        call([(np.zeros((3, A.NQ)), F64, (A.NQ,)), (np.zeros((2, A.NV)), F64, (A.NV,)), (np.zeros(3), F64, ())], None, [(None, F64, (A.NSTATE,))])


def test_the_methods_keep_their_own_rules_before_the_helper():
    b = Batch.__new__(Batch)                                          # no library, no device: these are refused before either is needed
    b.n, b.device = N_BATCH, 0
    with pytest.raises(ValueError):
        b.state_features(qpos=np.zeros((2, A.NQ)), qvel=np.zeros((2, A.NV)))
    with pytest.raises(ValueError):
        b.state_features(qpos=np.zeros((2, A.NQ)), qvel=np.zeros((2, A.NV)), phase=np.zeros(2), env_ids=[0, 1])
    with pytest.raises(ValueError):
        b.floor_contacts(qpos=np.zeros((2, A.NQ)), env_ids=[0, 1])
    with pytest.raises(ValueError):
        b.render(8, 8, rgb=False)
    with pytest.raises(ValueError):
        b.render(8, 8, qpos=np.zeros((1, A.NQ)), env_ids=[0])
    with pytest.raises(ValueError):
        b.render(8, 8, out={"rgb": np.zeros((N_BATCH, 8, 8, 4), dtype=np.uint8)})


# ---- csrc/view_stage.h on the host, under the sanitizers --------------------------------------------------------------------------------
def test_staging_layout_under_the_sanitizers(tmp_path):
    exe = HP.build_host("stage_host.cpp", tmp_path / "stage_host", sanitize=True, opt=("-O1", "-g"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    # 5 sizes x 2 callers x (2^7 + 2^5 + 2^3) presence masks of render, state features and floor contacts
    assert r.stdout.strip() == "stage_host: %d layouts hold" % (5 * 2 * (128 + 32 + 8)), r.stdout
