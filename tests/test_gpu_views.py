"""The staging the three read-only views share (csrc/views.hip Stage), on the GPU: one batch's staging buffer through a run of host-pointer
calls of different views and sizes, every result compared bit for bit with the same call on device tensors (which stage nothing); and a
refused call followed by a valid one.

The run of test_host_and_device_callers_agree_through_one_staging_buffer, in bytes of staging (regions at 256-byte steps; a view record is
1040 bytes): floor_contacts of 6 -> 256; state_features of 18 explicit states -> 5120 + 5120 + 256 + 24832 = 35328 (the buffer grows); render
8x8 of two environments with all four outputs -> 2304 records + 256 ids + 512 + 512 + 512 + 3072 = 7168 (six regions at six offsets inside
the larger buffer); floor_contacts of two ids -> 512; state_features of one id -> 256 + 1536."""
import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
N = 6
RENDER_KW = dict(depth=True, segmentation=True, geom_xform=True)


def stepped_batch(dtype):
    """6 environments set to varied states and stepped three times through host pointers"""
    mc = H.mocap("walk")
    b = Batch(H.compiled_model(), mc.data_config, mc.data_vel, N, device=0, mocap_dt=float(mc.dt), dtype=dtype)
    idx, q, v, _ws, _ctrl = H.varied_states(N, seed=21)
    b.set_state(q, v, frame_idx=idx)
    rng = np.random.RandomState(4)
    for _ in range(3):
        b.step(rng.randn(N, 28) * 0.9)
    return b


def kept_fields(b):
    return [b.get(f).copy() for f in (A.F_QPOS, A.F_QVEL, A.F_FRAME_IDX)]


def explicit_states():
    _idx, q, v, _ws, _ctrl = H.varied_states(18, seed=22)
    return q, v, np.linspace(0.0, 1.0, 18, endpoint=False)


def the_calls(b, device):
    """the five calls in order, on numpy arrays or on device tensors -> list of (name, result)"""
    conv = (lambda x: torch.as_tensor(x, device=DEV)) if device else (lambda x: x)
    q, v, ph = explicit_states()
    res = [("floor_contacts of all", b.floor_contacts(out=torch.zeros(N, dtype=torch.int32, device=DEV) if device else None))]
    res.append(("state_features of 18 states", b.state_features(qpos=conv(q), qvel=conv(v), phase=conv(ph))))
    img = b.render(8, 8, "side", env_ids=conv(np.array([4, 1], dtype=np.int32)), **RENDER_KW)
    res += [("render " + k, img[k]) for k in ("rgb", "depth", "segmentation", "geom_xform")]
    res.append(("floor_contacts of two ids", b.floor_contacts(env_ids=conv(np.array([5, 0], dtype=np.int32)))))
    res.append(("state_features of one id", b.state_features(env_ids=conv(np.array([2], dtype=np.int32)))))
    return res


@pytest.mark.parametrize("dtype", [64, 32])
def test_host_and_device_callers_agree_through_one_staging_buffer(dtype):
    hb, db = stepped_batch(dtype), stepped_batch(dtype)
    before = kept_fields(hb)
    for x, y in zip(before, kept_fields(db)):
        np.testing.assert_array_equal(x, y)                               # twins
    host = the_calls(hb, False)
    dev = the_calls(db, True)
    torch.cuda.synchronize()
    shapes = [(N,), (18, A.NSTATE), (2, 8, 8, 3), (2, 8, 8), (2, 8, 8), (2, A.NGEOM, 12), (2,), (1, A.NSTATE)]
    for (name, h), (_name, d), shp in zip(host, dev, shapes):
        assert isinstance(h, np.ndarray) and torch.is_tensor(d) and h.shape == shp == tuple(d.shape), name
        np.testing.assert_array_equal(h, d.cpu().numpy(), err_msg=name)
    res = dict(host)
    assert (res["render segmentation"] > 0).any() and np.isfinite(res["state_features of 18 states"]).all() and np.abs(res["render geom_xform"]).max() > 0.1
    # the subsets are rows of the whole: nothing was read at another call's offset
    np.testing.assert_array_equal(res["floor_contacts of two ids"], res["floor_contacts of all"][[5, 0]])
    np.testing.assert_array_equal(res["state_features of one id"], hb.state_features()[[2]])
    for b in (hb, db):
        for x, y in zip(before, kept_fields(b)):
            np.testing.assert_array_equal(x, y)                           # read-only
    hb.close(); db.close()


@pytest.mark.parametrize("ids_on_device", [True, False])
def test_a_refused_call_leaves_the_next_one_right(ids_on_device):
    b = stepped_batch(64)
    conv = (lambda x: torch.as_tensor(x, device=DEV)) if ids_on_device else (lambda x: x)
    host = lambda x: x.cpu().numpy() if torch.is_tensor(x) else x
    good, bad = np.array([3, 0], dtype=np.int32), np.array([3, N], dtype=np.int32)
    calls = {"dm_batch_floor_contacts": lambda ids: b.floor_contacts(env_ids=ids),
             "dm_batch_state_features": lambda ids: b.state_features(env_ids=ids),
             "dm_batch_render": lambda ids: b.render(8, 8, "side", env_ids=ids, **RENDER_KW)["geom_xform"]}
    want = {k: f(good).copy() for k, f in calls.items()}                  # (host pointers)
    for name, f in calls.items():
        for wrong in (bad, np.array([-1, 2], dtype=np.int32)):
            with pytest.raises(A.DmenvError, match="error -1: %s: env id out of range" % name):
                f(conv(wrong))
        np.testing.assert_array_equal(host(f(conv(good))), want[name], err_msg=name)
    np.testing.assert_array_equal(want["dm_batch_floor_contacts"], b.floor_contacts()[good])
    b.close()
