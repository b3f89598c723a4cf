"""Rendering without a GPU: the visual description, the float64 restatement of the scene and shading contract
(tests/render_numpy.py) against analytic cases, csrc/render.h built for the host against that restatement, tile_images and
the frame writer.  The GPU kernels are checked against the same restatement in tests/test_gpu_render.py."""
import os
import subprocess

import numpy as np
import pytest

from deepmimic_mujoco_amd import render as R
from deepmimic_mujoco_amd.humanoid import humanoid_visual
from deepmimic_mujoco_amd.mjcf import load_visual
from tests import helpers as H
from tests import render_numpy as RN
from tests.emu import hostprog as HP

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN_XML = os.path.join(ROOT, "tests", "golden", "dp_env_v3.xml")
CLIPS = ("walk", "spinkick", "dance_b")


def desc(cm, w, h, camera="side"):
    return RN.desc_dict(R.make_desc(cm, w, h, camera))


def test_builtin_visual_matches_the_xml():
    assert humanoid_visual() == load_visual(GOLDEN_XML)


def test_model_cameras_resolve_to_trackcom_offsets():
    cm = H.compiled_model()
    pos, mat, fovy, track = R.resolve_camera(cm, "side")
    assert track and fovy == 45.0
    xipos0 = cm.kinematics(cm.qpos0)[2]
    np.testing.assert_allclose(pos + R.subtree_com(cm, xipos0), [0.0, -3.0, 1.9], atol=1e-12)
    M = mat.reshape(3, 3)
    np.testing.assert_allclose(M.T @ M, np.eye(3), atol=1e-12)
    np.testing.assert_allclose(-M[:, 2], np.array([0.0, 2.0, -1.0]) / np.sqrt(5), atol=1e-12)   # looks along +y, down
    with pytest.raises(ValueError):
        R.resolve_camera(cm, "front")


def test_sphere_centre_lands_on_its_pinhole_pixel():
    cm = H.compiled_model()
    q = H.mocap("walk").data_config[5]
    d = desc(cm, 97, 61, "side")
    out = RN.render(cm, q, d)
    seen = 0
    for g in (1, 2, 3):                                       # root, chest, neck spheres
        p = out["gpos"][g] - out["cam"]
        M = d["cam_mat"]
        x, y, z = p @ M[:, 0], p @ M[:, 1], p @ M[:, 2]
        th = np.tan(np.radians(d["fovy"]) / 2)
        u, v = x / -z, y / -z
        c = int(np.floor(((u / (th * 97 / 61)) + 1) / 2 * 97)); r = int(np.floor((1 - v / th) / 2 * 61))
        # that geom's id, unless something nearer the camera covers the sphere's front there
        assert out["seg"][r, c] == g or out["depth"][r, c] < -z - cm.geom_size[g][0]
        seen += out["seg"][r, c] == g
    assert seen >= 2


def test_trackcom_camera_ignores_a_root_shift():
    cm = H.compiled_model()
    q = H.mocap("spinkick").data_config[10].copy()
    d = desc(cm, 64, 48, "back")
    a = RN.render(cm, q, d)
    q[0] += 3.7; q[1] -= 2.2
    b = RN.render(cm, q, d)
    body_a, body_b = a["seg"] > 0, b["seg"] > 0
    assert body_a.sum() > 50
    np.testing.assert_array_equal(body_a, body_b)
    np.testing.assert_array_equal(a["seg"][body_a], b["seg"][body_b])


def test_floor_depth_is_the_plane_distance():
    cm = H.compiled_model()
    cam = R.FreeCamera(lookat=(1.0, 2.0, 0.0), distance=6.0, azimuth=30.0, elevation=-35.0)
    d = RN.desc_dict(R.make_desc(cm, 64, 48, cam))
    q = cm.qpos0.copy(); q[0] = 30.0                          # the humanoid far out of view
    out = RN.render(cm, q, d)
    floor = out["seg"] == 0
    assert floor.mean() > 0.3
    pos, mat = out["cam"], d["cam_mat"]
    rays = RN.rays(d, mat)
    t = -pos[2] / rays[..., 2]
    np.testing.assert_allclose(out["depth"][floor], (t * -(rays @ mat[:, 2]))[floor], rtol=1e-12)
    # ... and the analytic one: the plane's distance along the optical axis, h / (n . -z) per unit of depth
    p = pos + t[..., None] * rays
    np.testing.assert_allclose(p[floor][:, 2], 0.0, atol=1e-9)


def test_checker_parity():
    cm = H.compiled_model()
    d = RN.desc_dict(R.make_desc(cm, 64, 64, R.FreeCamera(lookat=(0.25, 0.25, 0.0), distance=3.0, azimuth=0.0, elevation=-89.0)))
    q = cm.qpos0.copy(); q[0] = 30.0
    out = RN.render(cm, q, d)
    rays = RN.rays(d, d["cam_mat"])
    t = -out["cam"][2] / rays[..., 2]
    p = out["cam"] + t[..., None] * rays
    even = ((np.floor(p[..., 0] / 0.5) + np.floor(p[..., 1] / 0.5)) % 2 == 0) & (out["seg"] == 0)
    odd = ((np.floor(p[..., 0] / 0.5) + np.floor(p[..., 1] / 0.5)) % 2 == 1) & (out["seg"] == 0)
    assert even.sum() > 100 and odd.sum() > 100
    # rgb1 (.1 .2 .3) on even squares, rgb2 (.2 .3 .4) on odd ones: the blue channel tells them apart
    assert (out["rgb"][even][:, 2] < out["rgb"][odd][:, 2].min()).all()
    assert (out["parity"][even] == 0).all() and (out["parity"][odd] == 1).all()


def test_a_geom_above_a_floor_point_shadows_it():
    cm = H.compiled_model()
    q = cm.qpos0.copy()
    d = RN.desc_dict(R.make_desc(cm, 128, 128, R.FreeCamera(lookat=(0.0, 0.0, 0.3), distance=3.0, azimuth=0.0, elevation=-60.0)))
    out = RN.render(cm, q, d)
    rays = RN.rays(d, d["cam_mat"])
    t = -out["cam"][2] / rays[..., 2]
    p = out["cam"] + t[..., None] * rays
    floor = out["seg"] == 0
    # the light points straight down: a floor point lies in shadow when a sphere geom sits on the vertical line above it
    under = np.zeros(floor.shape, dtype=bool)
    for g in range(1, cm.ngeom):
        if cm.geom_type[g] == RN.SPHERE:
            under |= np.linalg.norm(p[..., :2] - out["gpos"][g][:2], axis=-1) < cm.geom_size[g][0] * 0.95
    assert (floor & under).sum() >= 3
    assert out["shadow"][floor & under].all()
    far = floor & (np.linalg.norm(p[..., :2] - out["gpos"][1][:2], axis=-1) > 1.2)
    assert far.sum() > 100 and not out["shadow"][far].any()
    lit = out["rgb"][floor & ~out["shadow"]].astype(int).sum(-1).min()
    dark = out["rgb"][floor & out["shadow"]].astype(int).sum(-1).max()
    assert dark < lit


# ---- csrc/render.h on the host ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def render_host(tmp_path_factory):
    out = HP.build_host("render_host.cpp", tmp_path_factory.mktemp("render_host") / "render_host", abi=True)
    return out


def host_render(exe, cm, views, tmp_path):
    """views: (qpos, descriptor dict) pairs -> [(rgb, depth, seg)] from csrc/render.h built for the host"""
    vals = [float(len(views))]
    for q, d in views:
        gpos, gmat, com = RN.geom_frames(cm, q)
        cam, mat = RN.camera(d, com)
        vals += [d["width"], d["height"]] + list(cam) + list(mat.reshape(9)) + [d["fovy"]] + list(d["geom_rgb"].reshape(48))
        vals += list(d["floor_rgb1"]) + list(d["floor_rgb2"]) + [d["floor_square"]] + list(d["sky_top"]) + list(d["sky_bottom"])
        vals += list(d["light_dir"]) + [d["ambient"], d["headlight"], d["diffuse"]] + list(cm.geom_size[0][:2]) + list(com)
        for g in range(cm.ngeom):
            vals += [float(cm.geom_type[g])] + list(gpos[g]) + list(gmat[g].reshape(9)) + list(cm.geom_size[g])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.asarray(vals, dtype=np.float64).tofile(fin)
    subprocess.check_call([exe, fin, fout])
    raw = np.fromfile(fout, dtype=np.uint8)
    res, o = [], 0
    for _q, d in views:
        W, H_ = d["width"], d["height"]
        n = W * H_
        rgb = raw[o:o + 3 * n].reshape(H_, W, 3); o += 3 * n
        depth = raw[o:o + 4 * n].view(np.float32).reshape(H_, W); o += 4 * n
        seg = raw[o:o + 4 * n].view(np.int32).reshape(H_, W); o += 4 * n
        res.append((rgb, depth, seg))
    assert o == raw.size
    return res


def cameras():
    return ["back", "side", R.FreeCamera(lookat=(0.0, 0.0, 0.3), distance=3.5, azimuth=135.0, elevation=-25.0, track_com=True)]


@pytest.mark.parametrize("size", [(64, 48), (97, 61)])
def test_render_h_on_the_host_matches_the_restatement(render_host, tmp_path, size):
    cm = H.compiled_model()
    views = []
    for clip in CLIPS:
        cfg = H.mocap(clip).data_config
        for f in (0, len(cfg) // 3, (2 * len(cfg)) // 3):
            for cam in cameras():
                views.append((cfg[f], RN.desc_dict(R.make_desc(cm, size[0], size[1], cam))))
    got = host_render(render_host, cm, views, tmp_path)
    failures = []
    for (q, d), (rgb, depth, seg) in zip(views, got):
        ref = RN.render(cm, q, d)
        for f in RN.compare(rgb, depth, seg, ref):
            failures.append(f)
        assert (seg > 0).sum() > 20                           # the body is in the picture
    assert not failures, failures[:10]


def test_tile_images_layout():
    imgs = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    t = R.tile_images(imgs)
    assert t.shape == (3 * 2, 2 * 3, 3)                        # ceil(sqrt(5)) = 3 rows of 2 tiles
    np.testing.assert_array_equal(t[0:2, 0:3], imgs[0])
    np.testing.assert_array_equal(t[0:2, 3:6], imgs[1])
    np.testing.assert_array_equal(t[2:4, 0:3], imgs[2])
    np.testing.assert_array_equal(t[4:6, 0:3], imgs[4])
    assert not t[4:6, 3:6].any()


def test_frame_writer_gif_and_npy(tmp_path):
    frames = [np.full((6, 8, 3), 40 * k, dtype=np.uint8) for k in range(4)]
    npy = R.write_frames(str(tmp_path / "a.npy"), frames)
    np.testing.assert_array_equal(np.load(npy), np.stack(frames))
    try:
        import PIL  # noqa: F401
    except ImportError:
        out = R.write_frames(str(tmp_path / "a.gif"), frames)
        assert out.endswith(".npy")
        return
    gif = R.write_frames(str(tmp_path / "a.gif"), frames, fps=10)
    assert gif.endswith(".gif")
    back = R.read_frames(gif)
    assert back.shape == (4, 6, 8, 3)
    np.testing.assert_array_equal(back[:, 0, 0, 0], [0, 40, 80, 120])
    with pytest.raises(ValueError):
        R.FrameWriter(str(tmp_path / "b.gif")).add(np.zeros((2, 2), dtype=np.uint8))
