"""dm_batch_render on the GPU (csrc/render_kernel.h): images against the float64 restatement (tests/render_numpy.py), geom frames
against CompiledModel.kinematics, bit-identical pairs of calls, no effect on the simulation, the gym / VecEnv facades, argument
checks and the two tools that write frames."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepmimic_mujoco_amd import _abi as A
from deepmimic_mujoco_amd import Batch, DPEnv, DPVecEnv
from deepmimic_mujoco_amd import render as R
from tests import helpers as H
from tests import render_numpy as RN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLIPS = ("walk", "spinkick", "dance_b")


def batch(n, dtype=64, clip="walk"):
    mc = H.mocap(clip)
    return Batch(H.compiled_model(), mc.data_config, mc.data_vel, n, device=0, mocap_dt=float(mc.dt), dtype=dtype)


def free_cam():
    return R.FreeCamera(lookat=(0.0, 0.0, 0.3), distance=3.5, azimuth=135.0, elevation=-25.0, track_com=True)


@pytest.mark.parametrize("dtype", [64, 32])
def test_images_match_the_restatement(dtype):
    cm = H.compiled_model()
    b = batch(1, dtype)
    failures, views = [], 0
    for clip in CLIPS:
        cfg = H.mocap(clip).data_config
        q = cfg[[0, len(cfg) // 4, len(cfg) // 2, (3 * len(cfg)) // 4]]
        for cam in ("back", "side", free_cam()):
            for W, Hh in ((64, 48), (97, 61), (320, 240)):
                out = b.render(W, Hh, cam, qpos=q, depth=True, segmentation=True)
                d = RN.desc_dict(R.make_desc(cm, W, Hh, cam))
                for k in range(len(q)):
                    ref = RN.render(cm, q[k], d)
                    f = RN.compare(out["rgb"][k], out["depth"][k], out["segmentation"][k], ref)
                    failures += ["%s frame %d %s %dx%d: %s" % (clip, k, cam, W, Hh, x) for x in f]
                    assert (out["segmentation"][k] > 0).sum() > 20
                    views += 1
    b.close()
    assert views == 108 and not failures, failures[:10]


@pytest.mark.parametrize("dtype,tol", [(64, 1e-12), (32, 1e-5)])
def test_geom_xform_matches_kinematics(dtype, tol):
    cm = H.compiled_model()
    b = batch(1, dtype)
    q = np.concatenate([H.mocap(c).data_config[::7] for c in CLIPS])
    q[:, 0] += np.linspace(-20, 20, len(q))                  # far from the origin too
    xf = b.render(8, 8, "side", qpos=q, rgb=False, geom_xform=True)["geom_xform"]
    for k in range(len(q)):
        gpos, gmat, _ = RN.geom_frames(cm, q[k])
        np.testing.assert_allclose(xf[k, :, :3], gpos, rtol=0, atol=tol * max(1.0, np.abs(gpos).max()))
        np.testing.assert_allclose(xf[k, :, 3:].reshape(16, 3, 3), gmat, rtol=0, atol=tol)
    b.close()


@pytest.mark.parametrize("dtype", [64, 32])
def test_bit_identical_pairs(dtype):
    n, W, Hh = 24, 97, 61
    b = batch(n, dtype, "spinkick")
    mc = H.mocap("spinkick")
    idx = (np.arange(n) * 3) % mc.data_config.shape[0]
    q, v = mc.data_config[idx].copy(), mc.data_vel[idx].copy()
    q[:, 0] += np.arange(n) * 0.5
    b.set_state(q, v)
    kw = dict(depth=True, segmentation=True)
    state = b.render(W, Hh, "back", **kw)
    qstate = b.get(A.F_QPOS)                                  # (the float32 library holds the state in float32)
    explicit = b.render(W, Hh, "back", qpos=qstate, **kw)
    ids = np.array([5, 0, 17, 17, 23], dtype=np.int32)
    sub = b.render(W, Hh, "back", env_ids=ids, **kw)
    one = b.render(W, Hh, "back", qpos=qstate[17:18], **kw)
    again = b.render(W, Hh, "back", **kw)
    dev_out = b.render(W, Hh, "back", out=dict(rgb=torch.empty((n, Hh, W, 3), dtype=torch.uint8, device=DEV),
                                              depth=torch.empty((n, Hh, W), dtype=torch.float32, device=DEV),
                                              segmentation=torch.empty((n, Hh, W), dtype=torch.int32, device=DEV)), **kw)
    torch.cuda.synchronize()
    for k in ("rgb", "depth", "segmentation"):
        a = state[k]
        assert np.array_equal(a, explicit[k]), k
        assert np.array_equal(a[ids], sub[k]), k
        assert np.array_equal(a[17:18], one[k]), k
        assert np.array_equal(a, again[k]), k
        assert np.array_equal(a, dev_out[k].cpu().numpy()), k
    assert (state["segmentation"] > 0).sum() > n * 50
    b.close()


def test_rendering_changes_nothing():
    n, T = 4096, 32
    rng = np.random.RandomState(5)
    acts = rng.randn(T, n, 28) * 0.9
    runs = []
    for with_render in (False, True):
        env = DPVecEnv(n, motion="walk", device=0, autoreset="rsi", seed=1, packed=True)
        env.reset()
        rec = []
        for t in range(T):
            obs, rew, done, _ = env.step(acts[t])
            rec.append((obs.copy(), rew.copy(), done.copy()))
            if with_render and t % 8 == 7:
                img = env.get_images(32, 24)
                assert img.shape == (n, 24, 32, 3)
        runs.append(rec)
        env.close()
    for (o0, r0, d0), (o1, r1, d1) in zip(*runs):
        assert np.array_equal(o0, o1) and np.array_equal(r0, r1) and np.array_equal(d0, d1)


def test_render_after_queued_steps_shows_the_post_step_state():
    n, T = 512, 6
    env = DPVecEnv(n, motion="walk", device=0, autoreset="rsi", seed=2, packed=True)
    env.reset()
    b = env.batch
    b.set_option(A.OPT_STEP_QUEUE, 16)
    before = b.render(48, 32, "side", segmentation=True)
    g = torch.Generator(device=DEV); g.manual_seed(3)
    ac = torch.randn((T, n, 28), generator=g, dtype=torch.float64, device=DEV) * 0.9
    ob = torch.zeros((T, n, 56), dtype=torch.float64, device=DEV); rew = torch.zeros((T, n), dtype=torch.float64, device=DEV)
    dn = torch.zeros((T, n), dtype=torch.uint8, device=DEV)
    for t in range(T):
        b.step(ac[t], 1, (ob[t], rew[t], dn[t]))
    assert b.queue_stats()[2] == T                            # queued, nothing launched yet
    img = b.render(48, 32, "side", segmentation=True)        # runs the queue first
    assert b.queue_stats()[2] == 0
    after = b.render(48, 32, "side", qpos=b.get(A.F_QPOS), segmentation=True)
    assert np.array_equal(img["rgb"], after["rgb"]) and np.array_equal(img["segmentation"], after["segmentation"])
    assert not np.array_equal(img["rgb"], before["rgb"])
    env.close()


def test_dpenv_and_vecenv_facades():
    env = DPEnv(motion="walk", device=0)
    env.reset()
    rgb = env.render("rgb_array", 80, 60)
    assert rgb.shape == (60, 80, 3) and rgb.dtype == np.uint8
    dep = env.render(mode="depth_array", width=80, height=60, camera_name="back")
    assert dep.shape == (60, 80) and dep.dtype == np.float32 and (dep > 0).all()
    assert dep[0].mean() > dep[-1].mean()                     # the camera looks down: the floor comes nearer towards the bottom rows
    up = env.render("depth_array", 80, 60, camera_name=R.FreeCamera(lookat=(0.0, 0.0, 1.0), distance=3.0, elevation=10.0, track_com=False))
    assert np.isinf(up[0]).all() and np.isfinite(up[-1]).all()   # sky at the top, floor at the bottom
    assert env.render("rgb_array").shape == (500, 500, 3)
    with pytest.raises(NotImplementedError):
        env.render()
    assert set(env.metadata["render.modes"]) == {"rgb_array", "depth_array"}
    env.close()
    venv = DPVecEnv(5, motion="walk", device=0)
    venv.reset()
    imgs = venv.get_images(40, 30, "side")
    assert imgs.shape == (5, 30, 40, 3) and imgs.dtype == np.uint8
    tiled = venv.render("rgb_array", 40, 30)
    assert tiled.shape == (3 * 30, 2 * 40, 3)
    np.testing.assert_array_equal(tiled, R.tile_images(imgs))
    with pytest.raises(NotImplementedError):
        venv.render("human")
    venv.close()


def test_invalid_arguments_raise():
    b = batch(4)
    with pytest.raises(ValueError):
        b.render(8, 8, "side", qpos=np.zeros((1, 35)), env_ids=[0])
    with pytest.raises(A.DmenvError):
        b.render(8, 8, "side", env_ids=np.array([0, 4], dtype=np.int32))
    with pytest.raises(A.DmenvError):
        b.render(8, 8, "side", env_ids=np.array([-1], dtype=np.int32))
    with pytest.raises(A.DmenvError):
        b.render(0, 8, "side")
    with pytest.raises(A.DmenvError):
        b.render(4097, 8, "side")
    L, h = b._L, b._h
    d = R.make_desc(b.compiled_model, 16, 16)
    buf = np.zeros(16 * 16 * 3, dtype=np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    q = np.tile(H.compiled_model().qpos0, (128, 1))
    ids = np.zeros(1, dtype=np.int32)
    assert L.dm_batch_render(h, None, None, 0, C.byref(d), p, None, None, None, A.PTR_HOST) == -1                   # n <= 0
    assert L.dm_batch_render(h, None, None, 5, C.byref(d), p, None, None, None, A.PTR_HOST) == -1                   # n > batch
    assert L.dm_batch_render(h, None, None, 1, C.byref(d), None, None, None, None, A.PTR_HOST) == -1                # no output
    assert L.dm_batch_render(h, C.c_void_p(q.ctypes.data), C.c_void_p(ids.ctypes.data), 1, C.byref(d), p, None, None, None, A.PTR_HOST) == -1
    big = R.make_desc(b.compiled_model, 4096, 4096)
    assert L.dm_batch_render(h, C.c_void_p(q.ctypes.data), None, 128, C.byref(big), p, None, None, None, A.PTR_HOST) == -1   # n W H = 2^31
    assert b"2^31" in L.dm_last_error()
    d.fovy = 0.0
    assert L.dm_batch_render(h, None, None, 1, C.byref(d), p, None, None, None, A.PTR_HOST) == -1
    b.close()


def _frames(path):
    return R.read_frames(path)


def test_play_mocap_tool_writes_changing_frames(tmp_path):
    out = str(tmp_path / "walk.gif")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "play_mocap.py"), "--motion", "walk", "--camera", "side", "--loops", "2",
                        "--width", "64", "--height", "48", "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    path = r.stdout.strip().split(" to ")[-1]
    f = _frames(path)
    assert f.shape == (2 * H.mocap("walk").data_config.shape[0], 48, 64, 3)
    assert np.abs(f[0].astype(int) - f[len(f) // 3].astype(int)).sum() > 0


def test_evaluate_render_out_writes_changing_frames(tmp_path):
    out = str(tmp_path / "eval.gif")
    ckpt = os.path.join(ROOT, "tests", "golden", "ckpt", "trpo-walk-0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_trpo.py"), "--task", "evaluate", "--load-model-path", ckpt,
                        "--number-trajs", "2", "--render-out", out, "--camera", "back", "--width", "48", "--height", "40"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("wrote ")][-1]
    f = _frames(line.split(" to ")[-1])
    assert f.ndim == 4 and f.shape[1:] == (40, 48, 3) and f.shape[0] >= 2
    assert np.abs(f[0].astype(int) - f[-1].astype(int)).sum() > 0
